// 32 x 32 output tile per workgroup, split-K over its 4 waves: the dense kernel for the layers that run ONCE PER FRAME on all
// object slots (M = B' N = 640 rows at cfg-2, K up to 1152, N up to 1152) and for their transposes in the backward pass.
//
// Why: with the 16 x 16 tile of k_linear every output tile re-reads 16 rows of activations and 16 columns of weights over the
// whole K: 0.125 operand bytes per MAC.  At 160 rows that is irrelevant (latency-bound); at 640 rows and up the launch is
// bound by what the L2s deliver (measured, tools/time_linear.py: time proportional to M, N and K, ~10 TB/s of operand
// traffic: 640 x 362 x 1152 13.4 us, its transpose 17.8 us).  A 32 x 32 tile halves the operand bytes per MAC; a wave's chunk
// (16 deep) feeds 2 A and 2 B fragments into 16 MFMAs.
//
// Structure: NW = 4, 8 or 16 waves split K, wave w owns chunks g = w + NW i.  Operand loads are issued in blocks of NB chunks,
// two blocks in flight (the loads of block b + 1 are issued before the MFMAs of block b); one accumulator per 16 x 16 tile,
// components x, y, z, w in four sweeps over the 4 independent accumulators; the waves' partial sums meet in LDS and the
// 64 NW threads finish the 1024 elements.  NW = 4 in production.  Per-wave stamps (tools/wave_lifetimes.py): a wave of the
// 4-wave version lives 11.2 us on 640 x 1152 x 384 for 3.9 us of matrix work -- one ~2.4 us round trip per block of 4 chunks --
// but cutting that chain with 8 or 16 waves per tile (one block each) is SLOWER (12.1 -> 30.9 us): every extra load in flight
// lengthens the round trips; the memory system's delivery to scattered 64-byte row pieces is the limit.
// Included twice by sqair_linear.hip / sqair_linear_dx.hip with SQ_T2_NAME / SQ_T2_DX set.
// Below kc = 40 the forward launcher does not come here: the widest of those launches (640 x 362 x 1152) goes to the one-round strip
// kernel of sqair_linear_strip.hip -- A resident in LDS, coalesced; B two chunks ahead behind UNCONDITIONAL loads (the `if` around
// SQ_T2_ISSUE below makes hipcc wait vmcnt(0) at the next use: the round trip per block this header describes) -- the others stay
// on k_linear.

// operand fetch of one block of NB chunks starting at this wave's chunk index `BASE` into register set SET
#define SQ_T2_ISSUE(SET, BASE)                                                                                     \
  _Pragma("unroll") for (int j = 0; j < NB; ++j) {                                                                 \
    const bool valid = (BASE) + j < nmine;                                                                         \
    const int g = valid ? wave + NW * ((BASE) + j) : 0;    /* beyond the end: chunk 0 against zero weights */   \
    const bool s1 = NSEG > 1 && g >= cum1, s2 = NSEG > 2 && g >= cum2, s3 = NSEG > 3 && g >= cum3;                  \
    const int cb = s3 ? cum3 : (s2 ? cum2 : (s1 ? cum1 : 0));                                                      \
    const int lim = s3 ? lim3 : (s2 ? lim2 : (s1 ? lim1 : lim0));                                                  \
    const int kk = min((g - cb) * 16 + kq * 4, lim);                                                               \
    a0##SET[j] = *reinterpret_cast<const f32x4*>((s3 ? rpa3 : (s2 ? rpa2 : (s1 ? rpa1 : rpa0))) + kk);             \
    a1##SET[j] = *reinterpret_cast<const f32x4*>((s3 ? rpb3 : (s2 ? rpb2 : (s1 ? rpb1 : rpb0))) + kk);             \
    b0##SET[j] = *(valid ? wq0 + (size_t)g * 64 : wz);                                                             \
    b1##SET[j] = *(valid ? wq1 + (size_t)g * 64 : wz);                                                             \
  }
#define SQ_T2_SWEEP(SET, C)                                                                                        \
  _Pragma("unroll") for (int j = 0; j < NB; ++j) {                                                                 \
    acc00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0##SET[j].C, b0##SET[j].C, acc00, 0, 0, 0);                      \
    acc01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0##SET[j].C, b1##SET[j].C, acc01, 0, 0, 0);                      \
    acc10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1##SET[j].C, b0##SET[j].C, acc10, 0, 0, 0);                      \
    acc11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1##SET[j].C, b1##SET[j].C, acc11, 0, 0, 0);                      \
  }
#define SQ_T2_MFMA(SET) SQ_T2_SWEEP(SET, x) SQ_T2_SWEEP(SET, y) SQ_T2_SWEEP(SET, z) SQ_T2_SWEEP(SET, w)

#ifndef SQ_T2_DX
template <int NB, int NSEG, int NW>
__global__ __launch_bounds__(64 * NW) void SQ_T2_NAME(const LinArgs a, const int kc_total, const int n_tiles SQ_TLP) {
#else
template <int NB, int NW>
__global__ __launch_bounds__(64 * NW) void SQ_T2_NAME(const DxArgs a, const int kc_total, const int n_tiles SQ_TLP) {
  constexpr int NSEG = 1;
#endif
  SQ_TL_SCOPE;
  __shared__ float red[NW * 4 * 256];   // [wave][tile (rt, ct)][256]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, kq = lane >> 4, l15 = lane & 15;
  const int tile_n = blockIdx.x * 2, tile_m = blockIdx.y * 2;
  const int arow_a = min(tile_m * 16 + l15, a.M - 1), arow_b = min(tile_m * 16 + 16 + l15, a.M - 1);
  int cum1 = 0x7fffffff, cum2 = 0x7fffffff, cum3 = 0x7fffffff;
#ifndef SQ_T2_DX
#define SQ_T2_ROW(sg, r) ((sg).rmul ? (int)__umulhi((unsigned)(r), (sg).rmul) : (r))
  const float* rpa0 = a.seg[0].p + (size_t)SQ_T2_ROW(a.seg[0], arow_a) * a.seg[0].ld;
  const float* rpb0 = a.seg[0].p + (size_t)SQ_T2_ROW(a.seg[0], arow_b) * a.seg[0].ld;
  const float *rpa1 = rpa0, *rpa2 = rpa0, *rpa3 = rpa0, *rpb1 = rpb0, *rpb2 = rpb0, *rpb3 = rpb0;
  int lim0 = ((a.seg[0].width + 3) & ~3) - 4, lim1 = 0, lim2 = 0, lim3 = 0;
  {
    int c = (a.seg[0].width + 15) >> 4;
    if (NSEG > 1 && a.nseg > 1) {
      cum1 = c; c += (a.seg[1].width + 15) >> 4; lim1 = ((a.seg[1].width + 3) & ~3) - 4;
      rpa1 = a.seg[1].p + (size_t)SQ_T2_ROW(a.seg[1], arow_a) * a.seg[1].ld; rpb1 = a.seg[1].p + (size_t)SQ_T2_ROW(a.seg[1], arow_b) * a.seg[1].ld;
    }
    if (NSEG > 2 && a.nseg > 2) {
      cum2 = c; c += (a.seg[2].width + 15) >> 4; lim2 = ((a.seg[2].width + 3) & ~3) - 4;
      rpa2 = a.seg[2].p + (size_t)SQ_T2_ROW(a.seg[2], arow_a) * a.seg[2].ld; rpb2 = a.seg[2].p + (size_t)SQ_T2_ROW(a.seg[2], arow_b) * a.seg[2].ld;
    }
    if (NSEG > 3 && a.nseg > 3) {
      cum3 = c; lim3 = ((a.seg[3].width + 3) & ~3) - 4;
      rpa3 = a.seg[3].p + (size_t)SQ_T2_ROW(a.seg[3], arow_a) * a.seg[3].ld; rpb3 = a.seg[3].p + (size_t)SQ_T2_ROW(a.seg[3], arow_b) * a.seg[3].ld;
    }
  }
#undef SQ_T2_ROW
#else
  const float* rpa0 = a.dpre + (size_t)arow_a * a.ld;
  const float* rpb0 = a.dpre + (size_t)arow_b * a.ld;
  const float *rpa1 = rpa0, *rpa2 = rpa0, *rpa3 = rpa0, *rpb1 = rpb0, *rpb2 = rpb0, *rpb3 = rpb0;
  const int lim0 = ((a.width + 3) & ~3) - 4, lim1 = 0, lim2 = 0, lim3 = 0;
#endif
  const f32x4* __restrict__ wq0 = reinterpret_cast<const f32x4*>(a.wp) + ((size_t)min(tile_n, n_tiles - 1) * kc_total) * 64 + lane;
  const f32x4* __restrict__ wq1 = reinterpret_cast<const f32x4*>(a.wp) + ((size_t)min(tile_n + 1, n_tiles - 1) * kc_total) * 64 + lane;
  const f32x4* __restrict__ wz = reinterpret_cast<const f32x4*>(a.wzero) + lane;
  const int nmine = (kc_total - wave + NW - 1) / NW;
  f32x4 acc00 = {0.0f, 0.0f, 0.0f, 0.0f}, acc01 = acc00, acc10 = acc00, acc11 = acc00;
  f32x4 a0P[NB], a1P[NB], b0P[NB], b1P[NB], a0Q[NB], a1Q[NB], b0Q[NB], b1Q[NB];
  SQ_T2_ISSUE(P, 0)
  // (keep every load of a block above the MFMAs of the previous one: the machine scheduler otherwise sinks each load to its use)
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll 1
  for (int base = 0; base < nmine; base += 2 * NB) {
    if (base + NB < nmine) { SQ_T2_ISSUE(Q, base + NB) }
    __builtin_amdgcn_sched_barrier(0);
    SQ_T2_MFMA(P)
    __builtin_amdgcn_sched_barrier(0);
    if (base + NB < nmine) {
      if (base + 2 * NB < nmine) { SQ_T2_ISSUE(P, base + 2 * NB) }
      __builtin_amdgcn_sched_barrier(0);
      SQ_T2_MFMA(Q)
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  // split-K reduction: component q of lane (kq, l15) of tile (rt, ct) is C[16 rt + 4 kq + q][16 ct + l15]
  float* r = red + wave * 1024 + (4 * kq) * 16 + l15;
  r[0 * 256 + 0] = acc00.x; r[0 * 256 + 16] = acc00.y; r[0 * 256 + 32] = acc00.z; r[0 * 256 + 48] = acc00.w;
  r[1 * 256 + 0] = acc01.x; r[1 * 256 + 16] = acc01.y; r[1 * 256 + 32] = acc01.z; r[1 * 256 + 48] = acc01.w;
  r[2 * 256 + 0] = acc10.x; r[2 * 256 + 16] = acc10.y; r[2 * 256 + 32] = acc10.z; r[2 * 256 + 48] = acc10.w;
  r[3 * 256 + 0] = acc11.x; r[3 * 256 + 16] = acc11.y; r[3 * 256 + 32] = acc11.z; r[3 * 256 + 48] = acc11.w;
  __syncthreads();
  // 64 NW threads finish the 4 tiles x 256 elements: element e = tid + 64 NW j -> tile q = e >> 8 (wave-uniform: 256 | 64 NW j
  // and a wave covers 64 consecutive elements of one tile), position p = e & 255 = (row p >> 4, column p & 15) of that tile
#pragma unroll
  for (int j = 0; j < 1024 / (64 * NW); ++j) {
    const int e = tid + 64 * NW * j;
    const int q = e >> 8, pq = e & 255, rt = q >> 1, ct = q & 1;
    const int m = (tile_m + rt) * 16 + (pq >> 4), n = (tile_n + ct) * 16 + (pq & 15);
    float sum = 0.0f;
#pragma unroll
    for (int w = 0; w < NW; ++w) sum += red[w * 1024 + q * 256 + pq];
#ifndef SQ_T2_DX
    if (tile_n + ct < n_tiles && m < a.M && n < a.N) {
      const bool use_add = a.add != nullptr && n < a.add_n;
      const bool g1 = a.epi == EPI_GRU1 && n >= a.nh && n < 2 * a.nh, g2 = a.epi == EPI_GRU2;
      float p_add = 0.0f, p_e0 = 0.0f, p_e1 = 0.0f;
      if (use_add) p_add = a.add[(size_t)(a.add_rmul ? (int)__umulhi((unsigned)m, a.add_rmul) : m) * a.add_ld + n];
      if (g1) p_e0 = a.e0[(size_t)m * a.e0_ld + (n - a.nh)];
      if (g2) { p_e0 = a.e0[(size_t)m * a.e0_ld + n]; p_e1 = a.e1[(size_t)m * a.e1_ld + n]; }
      const float p_scale = a.scale_ptr != nullptr ? *a.scale_ptr : 1.0f;
      x_epilogue(a, m, n, sum + a.bias[n] + p_add, p_e0, p_e1, p_scale);
    }
#else
    // the range of a column tile is wave-uniform (range starts are multiples of 16)
    const int n_tile0 = (tile_n + ct) * 16;
    int ri = 0;
    if (a.nranges > 1 && n_tile0 >= a.r[1].n0) ri = 1;
    if (a.nranges > 2 && n_tile0 >= a.r[2].n0) ri = 2;
    const DxRange rg = a.r[__builtin_amdgcn_readfirstlane(ri)];   // (scalar index, by value: one batch of scalar loads -- see k_linear_dx)
    if (tile_n + ct < n_tiles && m < a.M && n >= rg.n0 && n < rg.n1) {
      const int c = n - rg.n0;
      float v = sum * (a.scale_ptr != nullptr ? *a.scale_ptr : 1.0f);
      if (rg.add != nullptr) v += rg.add[(size_t)m * rg.add_ld + c];
      if (rg.saved != nullptr) v = dx_dact(v, rg.saved[(size_t)m * rg.saved_ld + c], c < rg.act_split ? rg.act_a : rg.act_b);
      rg.dst[(size_t)m * rg.dst_ld + c] = v;
      if (rg.dst2 != nullptr) rg.dst2[(size_t)m * rg.dst2_ld + c] = v;
    }
#endif
  }
}
#undef SQ_T2_ISSUE
#undef SQ_T2_SWEEP
#undef SQ_T2_MFMA
