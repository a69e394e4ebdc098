// Body of the dense-layer kernel; included by sqair_linear.hip (production, no knobs) and by
// tools/linear_floor.hip (ablation variants selected with SQ_ABL_* macros).
// NCH = K-chunks per wave handled per block of the (normally single-trip) chunk loop; the host picks
// the instantiation that covers ceil(kc / 4) so that all operand loads of a wave are in flight at once.
template <int NCH, int NSEG = 4, bool GRU = true>
__global__ __launch_bounds__(256) void SQ_KLINEAR_NAME(const float* __restrict__ p0, const float* __restrict__ wp0, const int ld0,
                                                const int width0, const unsigned rmul0, const int M0, const int kc_total,
                                                const int n_tiles, const float* __restrict__ wzero0, const LinArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  // The leading scalars repeat segment 0 / the weight pointer / M of `a`: scalar kernel arguments are eligible for
  // kernarg preloading into SGPRs (-mllvm -amdgpu-kernarg-preload-count), a by-value struct is not — with them the
  // single-segment instantiations issue every operand load before the s_load of the struct has returned (the block of
  // zero weights `wzero0` is among them for that reason; the epilogue operands, which do need the struct, are requested
  // AFTER the first block of operand loads and still ahead of the MFMAs).
  __shared__ float red[4 * 256];
  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
#if defined(SQ_ROWTILE_XCD_AFFINITY)  // (tools/linear_floor.hip only: measured, not used in production)
  // Row-tile -> XCD affinity: workgroup b runs on XCD b % 8 (observed dispatch order, a speed assumption only), so
  // every workgroup that touches row tile tm is placed on XCD tm % 8.  The activations a slot-loop layer reads
  // were then written on the same XCD by the previous layer and are still in that XCD's L2 (a cross-XCD read of
  // freshly written data measures ~1 us, an L2 hit ~0.3 us).  Grid = 8 * n_tiles * ceil(m_tiles / 8); surplus
  // workgroups exit at once.
  const int xcd = blockIdx.x & 7, qq = blockIdx.x >> 3;
  const int tile_n = qq % n_tiles;
  const int tile_m = xcd + 8 * (qq / n_tiles);
  if (tile_m * 16 >= a.M) return;
#else
  // 2-D grid (n-tile fastest in the linear block order, so a weight slab keeps its XCD) — no integer division
  const int tile_n = blockIdx.x;
  const int tile_m = blockIdx.y;
  (void)n_tiles;
#endif
  const int arow = min(tile_m * 16 + (lane & 15), M0 - 1);
  const int kq = lane >> 4;

  const f32x4* __restrict__ wp = reinterpret_cast<const f32x4*>(wp0) + ((size_t)tile_n * kc_total) * 64 + lane;
  const int nmine = (kc_total - wave + 3) >> 2;  // this wave owns global chunks g = wave + 4 i
  const f32x4* __restrict__ wz = reinterpret_cast<const f32x4*>(wzero0) + lane;
  f32x4 av[NCH], bv[NCH];
#ifdef SQ_ABL_NO_B
#define SQ_KL_LOADB(p) f32x4{1.0f, 1.0f, 1.0f, 1.0f}
#else
#define SQ_KL_LOADB(p) *(p)
#endif
  // Multi-segment layers: the weight blocks are requested HERE -- their addresses need nothing but the leading scalars, while the
  // activation addresses wait for the segment table (scalar loads of the argument struct + ~45 instructions per extra segment);
  // hipcc otherwise computes every address before it issues the first load, and a 4-segment layer requested its first operand
  // 225 instructions into the kernel.
#define SQ_KL_ISSUE_B(BASE)                                                                                      \
  _Pragma("unroll") for (int j = 0; j < NCH; ++j) {                                                              \
    const bool valid = (BASE) + j < nmine;                                                                       \
    const int g = valid ? wave + 4 * ((BASE) + j) : wave;                                                        \
    bv[j] = SQ_KL_LOADB(valid ? wp + (size_t)g * 64 : wz); /* invalid slots read the packed buffer's zero block */ \
  }
  // (Requesting the activation chunks of segment 0 here as well -- its row pointer and width are leading scalars too -- and
  // reloading only the chunks of the other segments once the table is known was measured: +0.08 ms on the forward step, the
  // conditional reloads sink next to their MFMAs.)
  if (NSEG > 1) {
    SQ_KL_ISSUE_B(0)
    __builtin_amdgcn_sched_barrier(0);
  }

  // ---- segment table (chunk ranges are wave-uniform)
  int cum1 = 0x7fffffff, cum2 = 0x7fffffff, cum3 = 0x7fffffff;
#define SQ_ROWOF(sg) ((sg).rmul ? (int)__umulhi((unsigned)arow, (sg).rmul) : arow)
  const float* rp0 = p0 + (size_t)(rmul0 ? (int)__umulhi((unsigned)arow, rmul0) : arow) * ld0;
  const float* rp1 = rp0; const float* rp2 = rp0; const float* rp3 = rp0;
  int lim0 = ((width0 + 3) & ~3) - 4, lim1 = 0, lim2 = 0, lim3 = 0;
  {
    int c = (width0 + 15) >> 4;
    if (NSEG > 1 && a.nseg > 1) { cum1 = c; c += (a.seg[1].width + 15) >> 4; rp1 = a.seg[1].p + (size_t)SQ_ROWOF(a.seg[1]) * a.seg[1].ld; lim1 = ((a.seg[1].width + 3) & ~3) - 4; }
    if (NSEG > 2 && a.nseg > 2) { cum2 = c; c += (a.seg[2].width + 15) >> 4; rp2 = a.seg[2].p + (size_t)SQ_ROWOF(a.seg[2]) * a.seg[2].ld; lim2 = ((a.seg[2].width + 3) & ~3) - 4; }
    if (NSEG > 3 && a.nseg > 3) { cum3 = c; rp3 = a.seg[3].p + (size_t)SQ_ROWOF(a.seg[3]) * a.seg[3].ld; lim3 = ((a.seg[3].width + 3) & ~3) - 4; }
  }

#undef SQ_ROWOF
  f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};
#ifdef SQ_ABL_NO_A
#define SQ_KL_LOADA(p) f32x4{1.0f, 1.0f, 1.0f, 1.0f}
#else
#define SQ_KL_LOADA(p) *reinterpret_cast<const f32x4*>(p)
#endif
// FIRST: the first block of a multi-segment layer (whose weight loads went out above); otherwise activations and weights together
#define SQ_KL_ISSUE(BASE, FIRST)                                                                                 \
  _Pragma("unroll") for (int j = 0; j < NCH; ++j) {                                                              \
    const bool valid = (BASE) + j < nmine;                                                                       \
    const int g = valid ? wave + 4 * ((BASE) + j) : wave; /* invalid slots re-read A chunk `wave` against zero weights */ \
    const bool s1 = NSEG > 1 && g >= cum1, s2 = NSEG > 2 && g >= cum2, s3 = NSEG > 3 && g >= cum3; /* wave-uniform */ \
    const float* rp = s3 ? rp3 : (s2 ? rp2 : (s1 ? rp1 : rp0));                                                  \
    const int cb = s3 ? cum3 : (s2 ? cum2 : (s1 ? cum1 : 0));                                                    \
    const int lim = s3 ? lim3 : (s2 ? lim2 : (s1 ? lim1 : lim0));                                                \
    av[j] = SQ_KL_LOADA(rp + min((g - cb) * 16 + kq * 4, lim));                                                  \
    if (!((FIRST) && NSEG > 1)) bv[j] = SQ_KL_LOADB(valid ? wp + (size_t)g * 64 : wz);                           \
  }
#ifndef SQ_ABL_NO_MFMA
#define SQ_KL_MFMA()                                                                                             \
  _Pragma("unroll") for (int j = 0; j < NCH; ++j) {                                                              \
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].x, bv[j].x, acc0, 0, 0, 0);                                \
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].y, bv[j].y, acc1, 0, 0, 0);                                \
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].z, bv[j].z, acc0, 0, 0, 0);                                \
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j].w, bv[j].w, acc1, 0, 0, 0);                                \
  }
#else
#define SQ_KL_MFMA() _Pragma("unroll") for (int j = 0; j < NCH; ++j) { acc0 += av[j] * bv[j]; }
#endif
  SQ_KL_ISSUE(0, true)
  __builtin_amdgcn_sched_barrier(0);  // (the scalar loads of the epilogue's struct fields must not be waited for above this line)
  // ---- epilogue operands: five unconditional loads (dummy = the bias word), requested right behind the first block of operand loads
  const int m = tile_m * 16 + (tid >> 4);
  const int n = tile_n * 16 + (tid & 15);
  const bool live = m < a.M && n < a.N;
  const int mc = min(m, a.M - 1), nc = min(n, a.N - 1);
  const float* pb = a.bias + nc;
  const bool use_add = a.add != nullptr && nc < a.add_n;
  const bool g1 = GRU && a.epi == EPI_GRU1 && nc >= a.nh && nc < 2 * a.nh;
  const bool g2 = GRU && a.epi == EPI_GRU2;
  const int mcd = a.add_rmul ? (int)__umulhi((unsigned)mc, a.add_rmul) : mc;
  const float* pa = use_add ? a.add + (size_t)mcd * a.add_ld + nc : pb;
  const float* pe0 = g1 ? a.e0 + (size_t)mc * a.e0_ld + (nc - a.nh) : (g2 ? a.e0 + (size_t)mc * a.e0_ld + nc : pb);
  const float* pe1 = g2 ? a.e1 + (size_t)mc * a.e1_ld + nc : pb;
  const float* psc = a.scale_ptr != nullptr ? a.scale_ptr : pb;
#ifdef SQ_ABL_NO_EPI
  const float p_bias = 0.0f; float p_add = 0.0f; const float p_e0 = 0.0f, p_e1 = 0.0f; float p_scale = 1.0f;
  (void)pa; (void)pe0; (void)pe1; (void)psc;
#else
  const float p_bias = *pb;
  float p_add = *pa;
  const float p_e0 = *pe0, p_e1 = *pe1;
  float p_scale = *psc;
#endif
  p_add = use_add ? p_add : 0.0f;
  p_scale = a.scale_ptr != nullptr ? p_scale : 1.0f;
  // the struct fields of the plain epilogue, fetched NOW (the empty asm pins them here): left to the compiler their scalar loads
  // sit between the barrier and the store, a scalar round trip on the tail of every launch
  const int e_split = a.act_split, e_acta = a.act_a, e_actb = a.act_b, e_ld = a.out_ld;
  float* const e_out = a.out;
  const float e_scale = a.scale;
  asm volatile("" ::"s"(e_split), "s"(e_acta), "s"(e_actb), "s"(e_ld), "s"(e_out), "s"(e_scale));

  // keep every load above every MFMA: left alone, the machine scheduler sinks each load next to its first use
  // (load, s_waitcnt vmcnt(0), mfma, load, ...), i.e. one memory round trip per chunk instead of one per kernel
  __builtin_amdgcn_sched_barrier(0);
  SQ_KL_MFMA()
  if (NCH == 10) {  // only the deepest instantiation loops (K > 640: the input encoder); the others cover their K in one block
#pragma unroll 1
    for (int base = NCH; base < nmine; base += NCH) {
      SQ_KL_ISSUE(base, false)
      __builtin_amdgcn_sched_barrier(0);
      SQ_KL_MFMA()
    }
  }
#undef SQ_KL_ISSUE
#undef SQ_KL_ISSUE_B
#undef SQ_KL_MFMA
#undef SQ_KL_LOADA
#undef SQ_KL_LOADB

#if defined(SQ_PREFETCH_NEXT_W)
  // experiment: pull the NEXT layer's weight slab `tile_n` (16 KB) into this XCD's L2 while this layer finishes
  // (a.e1 doubles as the pointer to the next layer's packed weights in the microbenchmark); results are never used
  if (a.e1 != nullptr) {
    const float* nw = a.e1 + ((size_t)tile_n * kc_total) * 256 + tid * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      f32x4 junk;
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(junk) : "v"(nw + (size_t)q * 1024 * (kc_total / 4)) : "memory");
    }
  }
#endif
  // split-K reduction: acc[i] of lane l is C[row = 4*(l>>4) + i][col = l & 15]
  float* r = red + wave * 256;
  r[(4 * kq + 0) * 16 + (lane & 15)] = acc0.x + acc1.x;
  r[(4 * kq + 1) * 16 + (lane & 15)] = acc0.y + acc1.y;
  r[(4 * kq + 2) * 16 + (lane & 15)] = acc0.z + acc1.z;
  r[(4 * kq + 3) * 16 + (lane & 15)] = acc0.w + acc1.w;
  __syncthreads();
  if (live) {
    float v = red[tid] + red[256 + tid] + red[512 + tid] + red[768 + tid] + p_bias + p_add;
    if (!GRU || a.epi == EPI_ACT) {
      v = sq_act(v, n < e_split ? e_acta : e_actb);
      e_out[(size_t)m * e_ld + n] = v * e_scale * p_scale;
    } else if (a.epi == EPI_GRU1) {
      // columns [z | r | x W_h + b_h]   (snt.GRU, SURVEY Appendix B)
      const int nh = a.nh;
      if (n < nh) a.out[(size_t)m * a.out_ld + n] = sq_sigmoid(v);
      else if (n < 2 * nh) {
        const float rg = sq_sigmoid(v);
        a.o1[(size_t)m * a.o1_ld + (n - nh)] = rg * p_e0;
        if (a.o3 != nullptr) a.o3[(size_t)m * a.o3_ld + (n - nh)] = rg;
      }
      else a.o2[(size_t)m * a.o2_ld + (n - 2 * nh)] = v;
    } else {  // EPI_GRU2: h' = (1 - z) h + z tanh(x W_h + (r h) U_h + b_h)
      const float hc = sq_tanh(v);
      a.out[(size_t)m * a.out_ld + n] = sq_gru_blend(p_e1, p_e0, hc);
      if (a.o1 != nullptr) a.o1[(size_t)m * a.o1_ld + n] = hc;
    }
  }
}

