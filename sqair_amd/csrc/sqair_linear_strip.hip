// One-round strip kernel for the widest once-per-frame dense layer on all object slots (cfg-2: 640 x 362 x 1152, 2880 workgroups
// of k_linear on 256 CUs): its own translation unit, so that the code object of sqair_linear.hip -- k_linear's size and placement,
// which the slot loop is sensitive to -- is the same with and without it.  Routed from sq_launch_linear (sq_launch_linear_strip).
//
// Why: with one 16 x 16 tile per workgroup every output tile re-reads 16 rows of A and 16 columns of B over the whole K, and a
// CU works through several rounds of workgroups; the time of those launches is proportional to (tiles per CU) x (K chunks),
// 0.047 us per (tile, chunk) = 2 KB of operand fetch -- what a CU can pull out of the L2s, 3.5 x the MFMA issue time.  Here a
// workgroup owns RT row tiles x a strip of G S adjacent column tiles, and the grid is ONE round of at most 256 workgroups:
//   * the workgroup is G GROUPS of 4 waves; a group is k_linear's four split-K waves for S of the strip's column tiles (all RT
//     row tiles).  G > 1 is what keeps a SIMD busy: with a lone wave per SIMD every instruction outside the MFMAs -- addresses,
//     the staging, the epilogue's activations -- issues at one per ~5 cycles with nothing to overlap it (the first version, one
//     group with the whole strip, took 14.2 us on 640 x 362 x 1152 against k_linear's 13.5 for 3.8 us of matrix work; three
//     groups of two tiles 11.0);
//   * the 16 RT rows of A (every segment of the LinArgs contract: pitch, width, row divisor, broadcast row, the clamp of a
//     ragged width) are fetched ONCE per workgroup, row-contiguously -- a wave instruction covers 1 KB of one row -- staged
//     through registers into an LDS image [row][16 kc + 4 floats] (the 4 floats of padding put the 16 rows of a fragment read on
//     distinct 16-byte slots), and stay there for the whole launch: a wave's fragment of chunk g is the ds_read_b128 at
//     (row = lane & 15, k = 16 g + 4 (lane >> 4)), the float4 k_linear loads from global memory.  (Register staging; LDS-DMA was
//     not measured);
//   * one barrier after the image is complete, none in the K loop;
//   * B comes straight from the packed slabs (fragment order, 1 KB contiguous per wave and chunk), two chunks ahead of the MFMAs
//     that consume it (three register sets, the order held with sched_barrier);
//   * arithmetic = k_linear's, bit for bit: wave w of a group owns chunks g = w + 4 i in order, per tile components x, z go into
//     acc0 and y, w into acc1, the partial is acc0 + acc1, and the four partials are summed as red[0] + red[1] + red[2] + red[3]
//     + bias + addend.  (Chunks beyond a wave's share multiply the pack's zero block, as in k_linear -- here up to the next
//     multiple of 3, there up to NCH: acc + x * 0 = acc whichever the count, an accumulator that starts at +0 is never -0.)  The
//     epilogue is x_epilogue's EPI_ACT path (the GRU layers are not routed here: they lost in the pass), with the activation
//     code a scalar where a tile lies on one side of act_split;
//   * after the K loop the image's space becomes the reduction buffer [group][wave][tile][256]; a thread sums its element of each
//     tile into slot [0], so that the epilogue proper (the activations' exp / log1p expansions) is ONE rolled loop body with
//     nothing indexed in registers.
// LDS: max(image, reduction buffer), dynamic: 47 KB at kc = 23, 80 KB at kc = 39 (launch_strip raises the kernel's limit).
// What it costs beyond the MFMAs is mostly CODE: a launch starts with a cold instruction cache, and the
// ~3 KB this kernel executes once (segment table, staging, operand addresses, epilogue) are worth 4 - 5 us -- more than the
// whole launch of the 256- and 400-column layers on k_linear, which is why only the widest layer comes here.
#include "sqair_common.h"
#include "sqair_lin_device.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define SQ_STRIP_KC_MAX 39      // deepest K (in chunks of 16) the route takes: from 40 on the 32 x 32 tile has the launch
#define SQ_STRIP_ROWS_MIN 512   // rows the route takes: [512, 768) -- cfg-2's 640-row launches; no other row count was measured
#define SQ_STRIP_ROWS_END 768
#define SQ_STRIP_GRID_MIN 192   // fewest workgroups of a strip launch (160, the 768-column GRU gate layer in strips of 6, lost)

template <int RT, int S, int G>
__global__ __launch_bounds__(256 * G) void k_linear_strip(const LinArgs a, const int kc_total, const int n_tiles SQ_TLP) {
  SQ_TL_SCOPE;
  static_assert(RT == 1 || RT == 2, "row tiles per workgroup");
  constexpr int NT = RT * S;                     // output tiles of a group
  constexpr int NR = (16 * RT + 4 * G - 1) / (4 * G);   // rows of the image a wave stages
  constexpr int NJ = (SQ_STRIP_KC_MAX * 4 + 63) / 64;   // 64-lane sweeps over a row's 16-byte units
  extern __shared__ __attribute__((aligned(16))) float lds[];   // max(image, reduction buffer): launch_strip sizes it
  const int lane = threadIdx.x & 63, kq = lane >> 4, l15 = lane & 15;
  const int wave_all = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // 0 .. 4 G - 1
  const int group = wave_all >> 2, wave = wave_all & 3;
  const int tid = threadIdx.x & 255;             // thread of the group
  const int tile_n0 = (blockIdx.x * G + group) * S, tile_m0 = blockIdx.y * RT;
  const int nmine = (kc_total - wave + 3) >> 2;  // this wave owns chunks g = wave + 4 i
  const int pitch = kc_total * 16 + 4;           // floats between rows of the image

  // ---- B: the first two chunks of every slab of the group are requested before anything else (surplus slabs of a ragged
  // strip re-read the last one; their sums are dropped)
  const f32x4* wq[S];
#pragma unroll
  for (int t = 0; t < S; ++t) wq[t] = reinterpret_cast<const f32x4*>(a.wp) + ((size_t)min(tile_n0 + t, n_tiles - 1) * kc_total) * 64 + lane;
  f32x4 bP[S], bQ[S], bR[S];
  const f32x4* __restrict__ wz = reinterpret_cast<const f32x4*>(a.wzero) + lane;
  // UNCONDITIONAL: a chunk beyond the wave's share reads the pack's zero block.  (Behind a branch -- even a wave-uniform one -- the
  // number of loads in flight is unknown to hipcc at the next use, and it waits for ALL of them, vmcnt(0), the ones just issued
  // included: one memory round trip per chunk.)
  // (Measured and dropped: ALL chunks of a wave requested in one burst up front, 8 or 12 register sets -- 640 x 362 x 1152
  // 11.0 -> 12.5 us, 640 x 312 x 768 8.2 -> 9.2: as sqair_linear_t2.inc found, more loads in flight only lengthen every round trip.)
#define SQ_ST_ISSUE(BV, I)                                                                        \
  {                                                                                               \
    const bool valid = (I) < nmine;                                                               \
    const size_t go = (size_t)(wave + 4 * (I)) * 64;                                              \
    _Pragma("unroll") for (int t = 0; t < S; ++t) BV[t] = *(valid ? wq[t] + go : wz);             \
  }
  SQ_ST_ISSUE(bP, 0)
  SQ_ST_ISSUE(bQ, 1)
  __builtin_amdgcn_sched_barrier(0);

  // ---- A: the image.  Wave w of the 4 G stages rows w, w + 4 G, .. of the 16 RT; lane l of sweep j takes the 16-byte unit
  // q = l + 64 j of the row: chunk q >> 2, floats 4 (q & 3) .. + 3 of it (the segment is a per-LANE choice here, the row a per-wave
  // one).  All loads of a wave go out before its first LDS store; addresses are clamped, not guarded.
  {
    const float* sp0 = a.seg[0].p; const float* sp1 = a.seg[1].p; const float* sp2 = a.seg[2].p; const float* sp3 = a.seg[3].p;
    const int sl0 = a.seg[0].ld, sl1 = a.seg[1].ld, sl2 = a.seg[2].ld, sl3 = a.seg[3].ld;
    const unsigned sm0 = a.seg[0].rmul, sm1 = a.seg[1].rmul, sm2 = a.seg[2].rmul, sm3 = a.seg[3].rmul;
    const int w0 = a.seg[0].width, w1 = a.seg[1].width, w2 = a.seg[2].width, w3 = a.seg[3].width;
    const int c1 = (w0 + 15) >> 4;
    const int c2 = c1 + (a.nseg > 1 ? (w1 + 15) >> 4 : 0);
    const int c3 = c2 + (a.nseg > 2 ? (w2 + 15) >> 4 : 0);
    const int cum1 = a.nseg > 1 ? c1 : 0x7fffffff, cum2 = a.nseg > 2 ? c2 : 0x7fffffff, cum3 = a.nseg > 3 ? c3 : 0x7fffffff;
    const int lim0 = ((w0 + 3) & ~3) - 4, lim1 = ((w1 + 3) & ~3) - 4, lim2 = ((w2 + 3) & ~3) - 4, lim3 = ((w3 + 3) & ~3) - 4;
    const int kc4 = kc_total * 4;
    int arow[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) arow[r] = min(tile_m0 * 16 + min(wave_all + 4 * G * r, 16 * RT - 1), a.M - 1);
    f32x4 st[NJ][NR];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (64 * j < kc4) {   // (wave-uniform)
        const int qc = min(lane + 64 * j, kc4 - 1);
        const int g = qc >> 2;
        const bool s1 = g >= cum1, s2 = g >= cum2, s3 = g >= cum3;
        const float* sp = s3 ? sp3 : (s2 ? sp2 : (s1 ? sp1 : sp0));
        const int sl = s3 ? sl3 : (s2 ? sl2 : (s1 ? sl1 : sl0));
        const unsigned sm = s3 ? sm3 : (s2 ? sm2 : (s1 ? sm1 : sm0));
        const int cb = s3 ? cum3 : (s2 ? cum2 : (s1 ? cum1 : 0));
        const int lim = s3 ? lim3 : (s2 ? lim2 : (s1 ? lim1 : lim0));
        const int kk = min((g - cb) * 16 + (qc & 3) * 4, lim);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const int rr = sm ? (int)__umulhi((unsigned)arow[r], sm) : arow[r];
          st[j][r] = *reinterpret_cast<const f32x4*>(sp + (size_t)rr * sl + kk);
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (64 * j < kc4) {
        const int q = lane + 64 * j;
        if (q < kc4) {
#pragma unroll
          for (int r = 0; r < NR; ++r)
            if ((16 * RT) % (4 * G) == 0 || wave_all + 4 * G * r < 16 * RT)   // (a wave count that does not divide the rows: wave-uniform)
              *reinterpret_cast<f32x4*>(&lds[(wave_all + 4 * G * r) * pitch + q * 4]) = st[j][r];
        }
      }
    }
  }
  // the image is complete: my LDS stores have landed (lgkmcnt(0)), then everybody's (the barrier).  No barrier from here until the
  // K loop is over.  (The two B chunks requested at the top HAVE landed by now: they are older than the staging loads, the vector
  // memory counter retires in order, and the last LDS store above waits vmcnt(0).  They cover their latency with the staging's, not
  // with the K loop; the loop's own prefetch starts with chunk 2.)
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_waitcnt(0xC07F);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);

  // ---- epilogue operands of this thread's element (row tid >> 4, column tid & 15) of every tile of the group, requested HERE,
  // ahead of the K loop that hides them: bursts of loads from clamped addresses, one wave-uniform branch around each burst; a
  // lane without the operand reads a word of the pack's zero block (NOT its bias word, as in k_linear: hipcc then loads the
  // operand into the bias word's register under a lane mask, and each burst waits for the one before); nothing looks at a value
  // before the loop is over
  const int er = tid >> 4, ec = tid & 15;
  const bool has_add = a.add != nullptr;
  float p_bias[NT], p_add[NT];
#define SQ_ST_NC(q) min(min(tile_n0 + (q) % S, n_tiles - 1) * 16 + ec, a.N - 1)
#define SQ_ST_MC(q) min((tile_m0 + (q) / S) * 16 + er, a.M - 1)
#pragma unroll
  for (int q = 0; q < NT; ++q) { p_bias[q] = a.bias[SQ_ST_NC(q)]; p_add[q] = 0.0f; }
  if (has_add) {
#pragma unroll
    for (int q = 0; q < NT; ++q) {
      const int nc = SQ_ST_NC(q), mc = SQ_ST_MC(q);
      const int mcd = a.add_rmul ? (int)__umulhi((unsigned)mc, a.add_rmul) : mc;
      p_add[q] = *(nc < a.add_n ? a.add + (size_t)mcd * a.add_ld + nc : a.wzero + ec);
    }
  }
  float p_scale = *(a.scale_ptr != nullptr ? a.scale_ptr : a.bias);
  __builtin_amdgcn_sched_barrier(0);

  f32x4 acc0[RT][S], acc1[RT][S];
#pragma unroll
  for (int r = 0; r < RT; ++r)
#pragma unroll
    for (int t = 0; t < S; ++t) { acc0[r][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f}; acc1[r][t] = acc0[r][t]; }
  const float* afrag = lds + l15 * pitch + kq * 4;
  // one chunk: the A fragments out of the image, then four sweeps over the RT S tiles
#define SQ_ST_SWEEP(BV, ACC, C)                                                                   \
  _Pragma("unroll") for (int r = 0; r < RT; ++r) {                                                \
    _Pragma("unroll") for (int t = 0; t < S; ++t)                                                 \
      ACC[r][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[r].C, BV[t].C, ACC[r][t], 0, 0, 0);     \
  }
#define SQ_ST_CONSUME(BV, I)                                                                      \
  {                                                                                               \
    f32x4 af[RT];                                                                                 \
    _Pragma("unroll") for (int r = 0; r < RT; ++r)                                                \
      af[r] = *reinterpret_cast<const f32x4*>(afrag + r * 16 * pitch + min(wave + 4 * (I), kc_total - 1) * 16); \
    SQ_ST_SWEEP(BV, acc0, x) SQ_ST_SWEEP(BV, acc1, y) SQ_ST_SWEEP(BV, acc0, z) SQ_ST_SWEEP(BV, acc1, w) \
  }
  // (keep the loads of chunk i + 2 above the MFMAs of chunk i: the machine scheduler otherwise sinks each load to its use)
#pragma unroll 1
  for (int i = 0; i < nmine; i += 3) {
    SQ_ST_ISSUE(bR, i + 2)
    __builtin_amdgcn_sched_barrier(0);
    SQ_ST_CONSUME(bP, i)
    __builtin_amdgcn_sched_barrier(0);
    SQ_ST_ISSUE(bP, i + 3)
    __builtin_amdgcn_sched_barrier(0);
    SQ_ST_CONSUME(bQ, i + 1)
    __builtin_amdgcn_sched_barrier(0);
    SQ_ST_ISSUE(bQ, i + 4)
    __builtin_amdgcn_sched_barrier(0);
    SQ_ST_CONSUME(bR, i + 2)
    __builtin_amdgcn_sched_barrier(0);
  }
#undef SQ_ST_ISSUE
#undef SQ_ST_SWEEP
#undef SQ_ST_CONSUME

  if (has_add) {
#pragma unroll
    for (int q = 0; q < NT; ++q) p_add[q] = SQ_ST_NC(q) < a.add_n ? p_add[q] : 0.0f;
  }
#undef SQ_ST_NC
#undef SQ_ST_MC
  p_scale = a.scale_ptr != nullptr ? p_scale : 1.0f;

  __syncthreads();   // every wave has read its last A fragment: the image's space becomes the reduction buffer
  // split-K reduction: acc[i] of lane l is C[row = 4 * (l >> 4) + i][col = l & 15]
  float* const red = lds + group * (4 * NT * 256);
  {
    float* r = red + wave * (NT * 256) + (4 * kq) * 16 + l15;
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
      for (int t = 0; t < S; ++t) {
        const int q = rt * S + t;
        r[q * 256 + 0] = acc0[rt][t].x + acc1[rt][t].x;
        r[q * 256 + 16] = acc0[rt][t].y + acc1[rt][t].y;
        r[q * 256 + 32] = acc0[rt][t].z + acc1[rt][t].z;
        r[q * 256 + 48] = acc0[rt][t].w + acc1[rt][t].w;
      }
    }
  }
  __syncthreads();
  // element (tile q, tid) of the group's four partial sums is read and written by thread tid alone from here on: its sum goes
  // back into slot [0]
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    float* e = red + q * 256 + tid;
    const float v = e[0] + e[NT * 256] + e[2 * NT * 256] + e[3 * NT * 256] + p_bias[q] + p_add[q];
    e[0] = v;
  }
#pragma unroll 1
  for (int q = 0; q < NT; ++q) {
    const int rt = q / S, t = q - rt * S;
    const int n0 = (tile_n0 + t) * 16;
    const int m = (tile_m0 + rt) * 16 + er, n = n0 + ec;
    if (tile_n0 + t < n_tiles && m < a.M && n < a.N) {
      const float* e = red + q * 256 + tid;
      // a tile on one side of act_split (all but one of a layer's, all of most layers'): the activation code is a SCALAR and
      // sq_act's switch one branch; a per-lane code runs all five cases under lane masks
      // (x_epilogue picks `n < act_split ? act_a : act_b`: handed a description whose two codes are the same, the choice folds)
      if (a.act_split <= n0) { LinArgs u = a; u.act_a = a.act_b; x_epilogue(u, m, n, e[0], 0.0f, 0.0f, p_scale); }
      else if (a.act_split >= n0 + 16) { LinArgs u = a; u.act_b = a.act_a; x_epilogue(u, m, n, e[0], 0.0f, 0.0f, p_scale); }
      else x_epilogue(a, m, n, e[0], 0.0f, 0.0f, p_scale);
    }
  }
}

// The launch of sq_launch_linear, if this kernel takes it (*taken; otherwise nothing has happened and the caller goes on to k_linear):
// EPI_ACT, 512 <= M < 768 rows, kc < 40, and ceil(mt / 2) x ceil(nt / 6) workgroups -- two row tiles x three groups of two column
// tiles each -- number 192 .. 256.  At 640 rows that is 55 .. 72 column tiles: the 1152-column layer (240 workgroups, 10.3 us
// busy in the pass against k_linear's 13.5) -- the ONE shape measured in the pass.  Everything else the predicate admits (513 ..
// 767 rows, other depths, 55 .. 90 column tiles) is taken by extrapolation from it: same workgroup count, same code executed once,
// K-loop work proportional to kc on both kernels.  No layer of the shipped configurations has such a shape; the unit tests do.  Measured and left on k_linear (tools/timeline.py, cfg-2, busy in the pass): the
// 768-column GRU gate layer in strips of 4 (240 workgroups of 8 waves) 9.3 us against 8.5; isolated (tools/wave_lifetimes.py) the
// 256-column layers in strips of 3 4.4 - 5.5 us against 2.8 - 4.1 and 128 -> 400 columns 4.9 against 2.45.
int sq_launch_linear_strip(const LinArgs& a, const PackedLayer& L, hipStream_t s, bool* taken) {
  constexpr int RT = 2, S = 2, G = 3;
  const int mt = (a.M + 15) / 16;
  const dim3 g((L.nt + G * S - 1) / (G * S), (mt + RT - 1) / RT);
  const int grid = (int)(g.x * g.y);
  *taken = a.epi == EPI_ACT && a.M >= SQ_STRIP_ROWS_MIN && a.M < SQ_STRIP_ROWS_END && L.kc <= SQ_STRIP_KC_MAX &&
           grid >= SQ_STRIP_GRID_MIN && grid <= 256;
  if (!*taken) return 0;
  const int image = 16 * RT * (16 * L.kc + 4) * 4, red = G * 4 * RT * S * 256 * 4;
  const int lds = image > red ? image : red;   // at most 32 x 628 floats = 80 KB (kc = 39)
  // the limit is raised ONCE per (kernel, device) -- sq_allow_big_lds remembers that it did, not to what -- so it is raised to the
  // route's ceiling, not to this launch's bytes: a first launch at kc = 32 would otherwise leave a later one at kc = 39 over it
  constexpr int LDS_CEILING = 16 * RT * (16 * SQ_STRIP_KC_MAX + 4) * 4;
  static_assert(LDS_CEILING <= 150 * 1024 && LDS_CEILING >= G * 4 * RT * S * 256 * 4, "the deepest image fits the CU's LDS and covers the reduction buffer");
  if (lds > 64 * 1024 && sq_allow_big_lds((const void*)k_linear_strip<RT, S, G>, LDS_CEILING) != 0) return -2;
  SQ_LAUNCH((k_linear_strip<RT, S, G>), g, dim3(256 * G), lds, s, a, L.kc, L.nt);
  return 0;
}
