// The packed dense operand: its layout, written down once (sq_pack_slot), and the planners that fill index tables in that layout.
// Host code that knows no handle: the product's plan (sqair_api.hip: build_layer, build_plan_T) and the dense unit-test entries
// (sqair_dense_test.hip) describe their layers in the vocabulary below and pack through the same functions.
#pragma once
#include "sqair_common.h"

// Float offset, inside a layer's pack of `kc` K chunks, of element (k, n): n the output column, k the row of the concatenated
// input with every segment padded to whole 16-row chunks.  This is the MFMA fragment order the k_linear family, the dX GEMM, the
// what-fusion layers and the slot chain read: tiles of 16 columns, per tile kc chunks of 64 lanes x 4 floats, lane =
// (k % 16 / 4) * 16 + n % 16, component k % 4.
SQ_LOCAL int64_t sq_pack_slot(int kc, int n, int k);

typedef std::vector<int> RowMap;  // per segment position: source row or -1
SQ_LOCAL RowMap rm_range(int start, int n);

// A layer's sources: per column block and segment a row-major matrix in the flat buffer (first element at `w`, leading dimension
// `ldw`; w < 0 = the segment feeds nothing into these columns) whose row rows[i] meets segment position i, columns col0 ..; the
// packed bias of column j of the block is flat[bias_a + col0 + j] + flat[bias_b + col0 + j] (< 0 = none).
struct PackSeg {
  int64_t w = -1;
  int ldw = 0;
  RowMap rows;
};
struct PackBlock {
  int ncols, col0;
  std::vector<PackSeg> seg;
  int64_t bias_a = -1, bias_b = -1;
};

// Index tables of a sequence of packed layers: per packed weight / bias element the index of its source in the flat buffer, or
// -1 (zero).  The weights start with a zero block: one K chunk of zero weights for the ragged tail of the kernels' chunk loop.
struct PackPlan {
  std::vector<int> widx = std::vector<int>(256, -1);
  std::vector<int> bidx_a, bidx_b;
  int64_t packed_w() const { return (int64_t)widx.size(); }
  int64_t packed_b() const { return (int64_t)bidx_a.size(); }
};

// Appends a layer of segments `seg_width` and the given column blocks to `p` (`id` names it in the abort() messages).
SQ_LOCAL PackedLayer sq_plan_layer(PackPlan& p, int id, const std::vector<int>& seg_width, const std::vector<PackBlock>& blocks);
// Appends to `dst` the transposed pack of layer L of `src` (which may be `dst`): dA_cat [M, 16 kc] = dPre [M, N] W^T with the same
// zero padding, so the gradient of a segment comes out in the segment's own order.  No bias.
SQ_LOCAL PackedLayer sq_plan_layer_T(PackPlan& dst, const PackPlan& src, const PackedLayer& L);
