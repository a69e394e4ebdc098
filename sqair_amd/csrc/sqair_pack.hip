// The packed dense operand's layout and its planners (sqair_pack.h).  Host code only.
#include "sqair_pack.h"

int64_t sq_pack_slot(int kc, int n, int k) {
  return ((((int64_t)(n / 16) * kc + k / 16) * 64) + ((k % 16) / 4) * 16 + n % 16) * 4 + k % 4;
}

RowMap rm_range(int start, int n) {
  RowMap r(n);
  for (int i = 0; i < n; ++i) r[i] = start + i;
  return r;
}

// a layer of kc chunks and N columns at the end of `p`, every source -1
static PackedLayer append_layer(PackPlan& p, int kc, int N, const std::vector<int>& seg_width) {
  PackedLayer L;
  L.seg_width = seg_width;
  L.kc = kc;
  L.N = N;
  L.nt = (N + 15) / 16;
  L.w_off = p.packed_w();
  L.b_off = p.packed_b();
  p.widx.resize(L.w_off + (int64_t)L.nt * L.kc * 256, -1);
  p.bidx_a.resize(L.b_off + L.nt * 16, -1);
  p.bidx_b.resize(L.b_off + L.nt * 16, -1);
  return L;
}

PackedLayer sq_plan_layer(PackPlan& p, int id, const std::vector<int>& seg_width, const std::vector<PackBlock>& blocks) {
  int kc = 0, N = 0;
  for (int w : seg_width) kc += (w + 15) / 16;
  for (const PackBlock& b : blocks) N += b.ncols;
  const PackedLayer L = append_layer(p, kc, N, seg_width);
  int n0 = 0;
  for (const PackBlock& b : blocks) {
    if (b.seg.size() != seg_width.size()) {
      fprintf(stderr, "sqair: layer %d: segment count mismatch\n", id);
      abort();
    }
    for (int j = 0; j < b.ncols; ++j) {
      const int n = n0 + j;
      if (b.bias_a >= 0) p.bidx_a[L.b_off + n] = (int)(b.bias_a + b.col0 + j);
      if (b.bias_b >= 0) p.bidx_b[L.b_off + n] = (int)(b.bias_b + b.col0 + j);
      int k0 = 0;   // first row of the segment in the chunk-padded concatenation
      for (size_t s = 0; s < seg_width.size(); ++s) {
        const PackSeg& src = b.seg[s];
        if (src.w >= 0) {
          if ((int)src.rows.size() != seg_width[s]) {
            fprintf(stderr, "sqair: layer %d seg %zu: rowmap %zu != width %d\n", id, s, src.rows.size(), seg_width[s]);
            abort();
          }
          for (int k = 0; k < seg_width[s]; ++k)
            if (src.rows[k] >= 0)
              p.widx[L.w_off + sq_pack_slot(L.kc, n, k0 + k)] = (int)(src.w + (int64_t)src.rows[k] * src.ldw + b.col0 + j);
        }
        k0 += (seg_width[s] + 15) / 16 * 16;
      }
    }
    n0 += b.ncols;
  }
  return L;
}

PackedLayer sq_plan_layer_T(PackPlan& dst, const PackPlan& src, const PackedLayer& L) {
  // reduction over the (padded) forward outputs, one output tile per forward K chunk
  const PackedLayer T = append_layer(dst, L.nt, L.kc * 16, {L.N});
  for (int k = 0; k < L.kc * 16; ++k)
    for (int n = 0; n < L.nt * 16; ++n) {
      const int from = src.widx[L.w_off + sq_pack_slot(L.kc, n, k)];
      if (from >= 0) dst.widx[T.w_off + sq_pack_slot(T.kc, k, n)] = from;
    }
  return T;
}
