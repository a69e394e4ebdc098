// Per-row spatial-transformer crop (k_crop_row).  The load flavour is a template parameter (plain loads in the product;
// an L1-bypassing flavour served the in-launch hand-off experiments of round 1).  Arithmetic order of the original
// per-sequence k_crop: results are bit-identical.
#pragma once
#include "sqair_glue.h"

typedef float sq_f32x4 __attribute__((ext_vector_type(4)));
struct LdPlain {
  static __device__ __forceinline__ float f(const float* p) { return *p; }
  static __device__ __forceinline__ sq_f32x4 f4(const float* p) { return *reinterpret_cast<const sq_f32x4*>(p); }
  static __device__ __forceinline__ void f4x4(const float* p0, const float* p1, const float* p2, const float* p3, sq_f32x4& v0,
                                              sq_f32x4& v1, sq_f32x4& v2, sq_f32x4& v3) {
    v0 = f4(p0); v1 = f4(p1); v2 = f4(p2); v3 = f4(p3);
    __builtin_amdgcn_sched_barrier(0);  // keep the loads above the MFMAs (see sqair_linear_kernel.inc)
  }
};

// One input of the transform's 8-wide output layer added to its eight running sums.  Outputs 0..5 take a fused multiply-add, outputs
// 6 and 7 (the raw scales of the last two `where` entries) a rounded product and then a rounded sum: that is how the compiler split
// the eight chains of `part[o] += x * w` between packed fma and packed multiply + add in the build that fixed the library's results
// (golden fixtures, the slot chain's restatement), so it is written out: every instantiation of the kernel gives these bits.
__device__ __forceinline__ void sq_tp_acc(float (&part)[8], const float x, const float4& wa, const float4& wb) {
  part[0] = __builtin_fmaf(x, wa.x, part[0]); part[1] = __builtin_fmaf(x, wa.y, part[1]);
  part[2] = __builtin_fmaf(x, wa.z, part[2]); part[3] = __builtin_fmaf(x, wa.w, part[3]);
  part[4] = __builtin_fmaf(x, wb.x, part[4]); part[5] = __builtin_fmaf(x, wb.y, part[5]);
  {
#pragma clang fp contract(off)
    const float p6 = x * wb.z, p7 = x * wb.w;
    part[6] = part[6] + p6;
    part[7] = part[7] + p7;
  }
}

template <class LD, bool stage_img>   // stage_img: the frame is copied to LDS (up to SQ_CROP_STAGE_MAX_PIXELS); else its taps are read where they lie
__device__ void x_crop_row(const CropArgs& a, const POff& po, const Dims& d, int r, int slot, float* smem) {
#define SQ_CROP_MODE a.mode
#define SQ_CROP_HAS_MASK (a.mask != nullptr)
#define SQ_CROP_FUSED_TP (a.t2 != nullptr && (a.mode == CROP_PROP2 || a.mode == CROP_DISC))
#include "sqair_crop_body.inc"
#undef SQ_CROP_MODE
#undef SQ_CROP_HAS_MASK
#undef SQ_CROP_FUSED_TP
}

// The specialised instantiation of one CropMode (sqair_glue.h: sq_spec_ok): the launch steps through its own mode only -- frame staged
// in LDS, with a mask unless it is a discovery crop, with the transform's output layer evaluated here (PROP2 / DISC) -- and the
// dimensions are constants.  Same expressions in the same order as the generic body: it IS the generic body.
template <class LD, int MODE>
__device__ void x_crop_row_spec(const CropArgs& a, const POff& po, const Dims& d_in, int r, int slot, float* smem) {
  constexpr bool stage_img = true;
  const Dims d = sq_spec_dims<true>(d_in);
#define SQ_CROP_MODE MODE
#define SQ_CROP_HAS_MASK (MODE != CROP_DISC)
#define SQ_CROP_FUSED_TP (MODE == CROP_PROP2 || MODE == CROP_DISC)
#include "sqair_crop_body.inc"
#undef SQ_CROP_MODE
#undef SQ_CROP_HAS_MASK
#undef SQ_CROP_FUSED_TP
}
