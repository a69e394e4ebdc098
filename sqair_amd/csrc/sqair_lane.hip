// The per-lane answers: the kernels that turn a lane's K particle rows into one answer per lane -- the SMC resampler, the forecast
// summaries, the lane estimate, the object layers, the stream score, the lane identities, the lane forecast, the lane tracks, the trajectory score of those two, the IDF1 table and the HOTA clip log with their solves.  None of them is a hop of the frame loop (once per pass or
// per call, on B workgroups), and they are a translation unit -- a code object -- of their own so that work on them moves no kernel of the pass
// (DESIGN.md section 3h).  Their compositions are the device functions of sqair_lane.h.  Every lane-wide sum is one thread's loop in
// index order: the same bits on every replay, and K <= 256 adds are nothing next to the pass.
#include "sqair_lane.h"
#include "sqair_canvas.h"

// ------------------------------------------------------------------------------------------------
// k_smc_resample (sqair_set_smc; SmcArgs in sqair_glue.h): the last launch of a pass with SMC on, after k_state_export.  Lane b's
// log weights a_k = log_w + this pass's per-frame log weights (frame order) -> ESS and the evidence, then either a systematic
// resampling written as the next pass's source map (k_state_import gathers the chosen rows out of the blob k_state_export just
// wrote) or the identity map with the weights carried on.
// ------------------------------------------------------------------------------------------------
constexpr unsigned SQ_SMC_PHILOX_TAG = 0x534D4352u;   // ("SMCR") counter word 1: never an element index of sqair_fill_noise
__global__ __launch_bounds__(256) void k_smc_resample(const SmcArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ float s_c[SQ_MAX_K];   // a_k, e_k, then the inclusive prefix c_k
  __shared__ SqLaneStats s_st;
  __shared__ float s_u;
  __shared__ int s_do;
  const int b = blockIdx.x, k = threadIdx.x, K = a.K, R = a.B * K, r = b * K + k;
  const float acc = k < K ? sq_lane_log_weight<false>(a.log_w, a.lw, a.T, R, r) : 0.0f;
  sq_lane_weights<true>(acc, K, s_c, s_st);
  if (k == 0) {
    const float m = s_st.m, c = s_st.S;
    const float ess = sq_lane_ess(c, s_st.Q), lse = m + logf(c / (float)K);
    const float lz = a.log_z[b];
    a.log_evidence[b] = lz + lse;
    a.ess[b] = ess;
    // (a NaN or infinite a_k, or every a_k at -inf, gives a non-finite ESS: such a lane never resamples, whatever ess_frac, so
    //  the identity map and the carried a_k keep the bad values where the caller can see them)
    const int go = isfinite(ess) && (a.ess_frac == 1.0f || ess < a.ess_frac * (float)K);
    float u;   // (drawn whether or not the lane resamples: u_out always holds this pass's u)
    if (a.uniforms != nullptr) {
      u = a.uniforms[b];
    } else {
      const unsigned ctr = (unsigned)(a.t_row[b * K] + a.T);   // (the lane's frame counter after the pass)
      unsigned w[4];
      philox4x32_10((unsigned)b, SQ_SMC_PHILOX_TAG, ctr, 0u, (unsigned)a.seed, (unsigned)(a.seed >> 32), w);
      u = (float)(w[0] >> 8) * (1.0f / 16777216.0f);   // [0, 1), 24 bits
    }
    if (a.u_out != nullptr) a.u_out[b] = u;
    if (go) a.log_z[b] = lz + lse;
    a.resampled[b] = go;
    s_u = u; s_do = go;
  }
  __syncthreads();
  if (k >= K) return;
  if (s_do) {
    // output k: the smallest i with c_i > (k + u) S / K.  If none (fp32 rounding of (k + u) S / K up to S = c_{K-1}: k = K - 1
    // and u near 1), the smallest i with c_i >= S, i.e. the last particle of positive weight, never a zero-weight one after it.
    // The predicate is monotone in i and true at K - 1; below S it is c_i > thr alone.
    const float thr = ((float)k + s_u) * s_st.S / (float)K, S = s_st.S;
    int lo = 0, hi = K - 1;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (s_c[mid] > thr || s_c[mid] >= S) hi = mid;
      else lo = mid + 1;
    }
    a.src[r] = b * K + lo;
    a.log_w[r] = 0.0f;
  } else {
    a.src[r] = r;
    a.log_w[r] = acc;
  }
}
int sq_launch_smc_resample(const SmcArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_smc_resample, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Forecasts (sqair_forecast, sqair_forecast_fan; include/sqair_hip.h states the semantics; the argument blocks: sqair_glue.h)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_forecast_fan_src(const int* __restrict__ src, int* __restrict__ src_fan, const int R, const int S SQ_TLP) {
  SQ_TL_SCOPE;
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= (long long)R * S) return;
  const int r = (int)(q / S);
  int sr = src != nullptr ? src[r] : r;
  if (sr < 0 || sr >= R) sr = -1;   // (the import's range rule against the blob's R: the fanned-out import never reads outside it)
  src_fan[q] = sr;
}
int sq_launch_forecast_fan_src(const int* src, int* src_fan, int R, int S, hipStream_t s) {
  const long long n = (long long)R * S;
  SQ_LAUNCH(k_forecast_fan_src, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, src_fan, R, S);
  return 0;
}
// Predictive summaries (ForecastSummaryArgs): workgroup (b, f).  The lane's weights, expanded to one weight per rollout row,
// w_q = w_{q / S} / S (S = 1: w_q = w_k, the division by 1.0f is exact), then both sums as loops over the lane's K*S rows.  A NaN or
// +inf weight, or all of them -inf, makes S -- and so every w_q -- NaN.
__global__ __launch_bounds__(256) void k_forecast_summary(const ForecastSummaryArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ float s_k[SQ_MAX_K];
  __shared__ float s_w[SQAIR_FORECAST_FAN_MAX];
  __shared__ SqLaneStats s_st;
  const int b = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, K = a.K, S = a.S, N = a.N, P = a.P, KS = K * S;
  const size_t row0 = ((size_t)f * a.B + b) * KS;   // (frame f, rollout 0 of lane b)
  sq_lane_weights<false>(tid < K ? sq_lane_log_weight<true>(a.log_w, nullptr, 0, a.B * K, b * K + tid) : 0.0f, K, s_k, s_st);
  for (int q = tid; q < KS; q += 256) s_w[q] = s_k[q / S] / (float)S;
  __syncthreads();
  if (tid == 0 && a.expected_count) {
    float cnt = 0.0f;
    for (int q = 0; q < KS; ++q) {
      float n = 0.0f;
      for (int j = 0; j < N; ++j) n += a.rec[((row0 + q) * N + j) * rec::W + rec::PRES];
      cnt += s_w[q] * n;
    }
    a.expected_count[(size_t)f * a.B + b] = cnt;
  }
  if (!a.mean_canvas) return;
  for (int p = tid; p < P; p += 256) a.mean_canvas[((size_t)f * a.B + b) * P + p] = sq_lane_mean_pixel(s_w, a.canvas, row0, P, p, KS);
}
int sq_launch_forecast_summary(const ForecastSummaryArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_forecast_summary, dim3(a.B, a.F), dim3(256), 0, s, a);
  return 0;
}

// The start body of the lane forecast and of the lane tracks: workgroup = lane b.  The weights and the best row, the best START
// row's objects and boxes, then thread k < K associates its particle's start row with them and leaves in the scratch, per (k, j),
// whether k is associated and the obj_id word it is followed by -- every step k_lane_estimate's, by the same functions.  TRACK: the
// start rows are the newest traced frame and carry a mask, `valid` [R]: an invalid row holds no objects and is associated with
// nothing.  Returns, for the kernel's own epilogue, the lane's best particle (-1: a non-finite lane) and, to thread j < N, whether
// best-row slot j is present.
struct SqLaneStart { int best; int present; };
template <bool TRACK>
__device__ __forceinline__ SqLaneStart sq_lane_start(const ForecastLaneArgs& a, const int* __restrict__ valid) {
  __shared__ float s_w[SQ_MAX_K];        // a_k, e_k, then w_k
  __shared__ unsigned char s_match[SQ_MAX_K * SQ_MAXN];
  __shared__ SqBox s_bbox[SQ_MAXN];      // the best start row's boxes
  __shared__ int s_bp[SQ_MAXN];          // ... and which of its slots are present
  __shared__ SqLaneStats s_st;
  const SqairForecastLane& o = a.lane;
  const LaneRows& v = a.start;
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, N = a.N, R = a.B * K, r = b * K + tid;
  // ---- 1: weights and the best row
  sq_lane_weights<false>(tid < K ? sq_lane_log_weight<true>(a.log_w, nullptr, 0, R, r) : 0.0f, K, s_w, s_st);
  const bool bad = s_st.best < 0;
  if (tid == 0) o.best_row[b] = bad ? -1 : b * K + s_st.best;
  if (tid < K) {
    a.x.w[r] = s_w[tid];
    if (o.weights) o.weights[r] = s_w[tid];
  }
  // ---- 2: the start records of the lane's rows (words copied), the best start row's objects and their boxes
  if (!TRACK)
    for (int i = tid; i < K * N; i += 256) {
      const int k = i / N;
      const size_t src = sq_lane_slot(v, (size_t)(b * K + k), N) + (i - k * N), dst = (size_t)b * K * N + i;
      if (o.start_presence) sq_put(o.start_presence + dst, sq_word(v.presence + src * v.pres_ld));
      if (o.start_obj_id) sq_put(o.start_obj_id + dst, sq_word(v.obj_id + src * v.id_ld));
      if (o.start_where)
        for (int c = 0; c < 4; ++c) sq_put(o.start_where + dst * 4 + c, sq_word(v.where + src * v.where_ld + c));
    }
  const size_t best = (size_t)(b * K + (bad ? 0 : s_st.best));
  sq_lane_best_objects(v, best, bad || (TRACK && !valid[best]), N, a.H, a.W, (size_t)b * N, SqBestOut{o.presence, o.obj_id, nullptr, o.box0},
                       s_bp, s_bbox);
  if (tid < N) a.x.bp[(size_t)b * N + tid] = s_bp[tid];
  // ---- 3: thread k's particle: per best-row object its first present start slot of maximal IoU, and that slot's id word
  if (tid < K) {
    if (TRACK && !valid[r]) {
      for (int j = 0; j < N; ++j) { s_match[tid * N + j] = 255; a.x.fm[(size_t)r * N + j] = 0; a.x.fid[(size_t)r * N + j] = 0u; }
    } else {
      sq_lane_associate<true>(v, (size_t)r, N, a.H, a.W, o.iou_min, s_bp, s_bbox, s_match + tid * N, a.x.fm + (size_t)r * N,
                              a.x.fid + (size_t)r * N);
    }
  }
  __syncthreads();
  if (tid < N && o.support) {
    const int j = tid;
    float sup = 0.0f;
    for (int k = 0; k < K; ++k) {
      if (s_match[k * N + j] == 255) continue;
      sup += s_w[k];
    }
    o.support[(size_t)b * N + j] = s_bp[j] ? sup : (bad ? __builtin_nanf("") : 0.0f);
  }
  return SqLaneStart{bad ? -1 : s_st.best, tid < N ? s_bp[tid] : 0};
}
__global__ __launch_bounds__(256) void k_forecast_lane_start(const ForecastLaneArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_start<false>(a, nullptr);
}
// The frame body of both: workgroup (lane b, frame f), thread = rollout q of the lane (K*S <= SQAIR_FORECAST_FAN_MAX: up to four per
// thread).  The rollouts' counts give count_prob; per object j each associated rollout looks its followed id up among its present
// slots and stages that slot's pixel box in LDS (16 bytes per rollout), then threads c < 4 reduce coordinate c in two passes, each
// ONE thread's loop over q in index order.  No per-thread arrays: nothing to spill.  TRACK (S = 1: rollout q = particle k's traced
// row of frame f): a row with valid[q] == 0 counts nowhere -- not in count_prob, not as a hit -- and valid_mass is the weight left.
template <bool TRACK>
__device__ __forceinline__ void sq_lane_frame(const ForecastLaneArgs& a, const int* __restrict__ valid, float* valid_mass) {
  constexpr unsigned char INVALID = 255;                // (a count is at most N <= 16)
  __shared__ float s_w[SQ_MAX_K];                       // w_k / S
  __shared__ SqBox s_stage[SQAIR_FORECAST_FAN_MAX];     // the box followed in rollout q
  __shared__ unsigned char s_hit[SQAIR_FORECAST_FAN_MAX];
  __shared__ unsigned char s_n[SQAIR_FORECAST_FAN_MAX];
  const SqairForecastLane& o = a.lane;
  const int b = blockIdx.x, f = blockIdx.y, tid = threadIdx.x, K = a.K, S = a.S, N = a.N, KS = K * S;
  const size_t fb = (size_t)f * a.B + b, row0 = fb * KS;   // (frame f, rollout 0 of lane b)
  const bool bad = o.best_row[b] < 0;
  const float nan = __builtin_nanf("");
  if (tid < K) s_w[tid] = a.x.w[b * K + tid] / (float)S;
  for (int q = tid; q < KS; q += 256) {
    int n = 0;
    for (int m = 0; m < N; ++m) n += a.presence[((row0 + q) * N + m) * a.pres_ld] != 0.0f ? 1 : 0;
    s_n[q] = TRACK && !valid[row0 + q] ? INVALID : (unsigned char)n;
  }
  __syncthreads();
  if (tid <= N && o.count_prob) {
    float p = 0.0f;
    for (int k = 0, q = 0; k < K; ++k) {
      const float w = s_w[k];
      for (int s = 0; s < S; ++s, ++q) p += s_n[q] == tid ? w : 0.0f;
    }
    o.count_prob[fb * (N + 1) + tid] = bad ? nan : p;
  }
  if (TRACK && tid == N + 1 && valid_mass) {
    float p = 0.0f;
    for (int k = 0; k < K; ++k) p += s_n[k] != INVALID ? s_w[k] : 0.0f;
    valid_mass[fb] = bad ? nan : p;
  }
  if (!o.alive && !o.box_mean && !o.box_std) return;
  for (int j = 0; j < N; ++j) {   // (the loop and its branches are uniform over the workgroup)
    const size_t e = fb * N + j;
    if (!a.x.bp[b * N + j]) {     // absent: zero (a non-finite lane: NaN)
      const float v = bad ? nan : 0.0f;
      if (tid == 0 && o.alive) o.alive[e] = v;
      if (tid < 4 && o.box_mean) o.box_mean[e * 4 + tid] = v;
      if (tid < 4 && o.box_std) o.box_std[e * 4 + tid] = v;
      continue;
    }
    for (int q = tid; q < KS; q += 256) {
      const size_t kj = (size_t)(b * K + q / S) * N + j;
      int hit = 0;
      if (a.x.fm[kj] && !(TRACK && s_n[q] == INVALID)) {
        const unsigned idw = a.x.fid[kj];
        for (int m = 0; m < N && !hit; ++m) {
          const size_t sl = (row0 + q) * N + m;
          if (a.presence[sl * a.pres_ld] != 0.0f && sq_word(a.obj_id + sl * a.id_ld) == idw) {
            s_stage[q] = sq_box_of_where(a.where + sl * a.where_ld, a.H, a.W);
            hit = 1;
          }
        }
      }
      s_hit[q] = (unsigned char)hit;
    }
    __syncthreads();
    if (tid < 4) {
      float al, sum;
      sq_lane_box_sum(s_w, s_stage, K, S, tid, [&](int q) { return s_hit[q] != 0; }, al, sum);
      const float mean = sum / al;
      float var = 0.0f;
      for (int k = 0, q = 0; k < K; ++k) {
        const float w = s_w[k];
        for (int s = 0; s < S; ++s, ++q) {
          if (!s_hit[q]) continue;
          const float dv = sq_box_coord(s_stage[q], tid) - mean;
          var += w * (dv * dv);
        }
      }
      if (tid == 0 && o.alive) o.alive[e] = al;
      if (o.box_mean) o.box_mean[e * 4 + tid] = mean;
      if (o.box_std) o.box_std[e * 4 + tid] = sqrtf(var / al);
    }
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_forecast_lane_frame(const ForecastLaneArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_frame<false>(a, nullptr, nullptr);
}
int sq_launch_forecast_lane(const ForecastLaneArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_forecast_lane_start, dim3(a.B), dim3(256), 0, s, a);
  SQ_LAUNCH(k_forecast_lane_frame, dim3(a.B, a.F), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Lane tracks (sqair_history_trace_lane; TrackLaneArgs in sqair_glue.h; the semantics: include/sqair_hip.h, points 1-8): the lane
// forecast's bodies over the traced rows, frame F - 1 standing where the forecast's start rows stand.
// ------------------------------------------------------------------------------------------------
// k_track_lane_start: workgroup = lane b.  After the shared body, thread j < N walks the best row's own path back from frame F - 1
// for as long as it is valid and holds object j's id word in a present slot: first_frame.
__global__ __launch_bounds__(256) void k_track_lane_start(const TrackLaneArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  const ForecastLaneArgs& g = a.f;
  const int b = blockIdx.x, j = threadIdx.x, N = g.N;
  const size_t R = (size_t)g.B * g.K;
  const SqLaneStart st = sq_lane_start<true>(g, a.valid + (size_t)(g.F - 1) * R);
  if (j >= N || !a.first_frame) return;
  int first = -1;
  if (st.present) {
    const size_t best = (size_t)b * g.K + st.best;
    const unsigned idw = sq_word(g.obj_id + (((size_t)(g.F - 1) * R + best) * N + j) * g.id_ld);
    for (int f = g.F - 1; f >= 0; --f) {
      const size_t row = (size_t)f * R + best;
      if (!a.valid[row]) break;
      bool has = false;
      for (int m = 0; m < N && !has; ++m) {
        const size_t sl = row * N + m;
        has = g.presence[sl * g.pres_ld] != 0.0f && sq_word(g.obj_id + sl * g.id_ld) == idw;
      }
      if (!has) break;
      first = f;
    }
  }
  a.first_frame[(size_t)b * N + j] = first;
}
// k_track_lane_frame: workgroup (lane b, frame f), thread k = the lane's traced row k of frame f
__global__ __launch_bounds__(256) void k_track_lane_frame(const TrackLaneArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_frame<true>(a.f, a.valid, a.valid_mass);
}
int sq_launch_track_lane(const TrackLaneArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_track_lane_start, dim3(a.f.B), dim3(256), 0, s, a);
  SQ_LAUNCH(k_track_lane_frame, dim3(a.f.B, a.f.F), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Lane estimates (sqair_set_estimate; LaneEstArgs in sqair_glue.h; the semantics: include/sqair_hip.h, points 1-8)
// ------------------------------------------------------------------------------------------------
// k_lane_estimate: workgroup (lane b, frame t, pixel chunk z).  Every workgroup forms the lane's weights at frame t; chunk z = 0 also
// gives the lane's answer:
//   thread k < K   its particle: n_k, and its association with the <= N best-row boxes in LDS, left as a K x N table of bytes;
//   per object j   the K matched boxes are recomputed by their threads into a 4 KB stage (K x N boxes would be 64 KB), then
//                  threads c < 4 reduce coordinate c, and the support, over k in index order.
// Nothing is accumulated with atomics.  CANVAS: the instantiation that also averages the canvases (est.mean_canvas set); the other
// one carries none of it.
template <bool CANVAS>
__global__ __launch_bounds__(256) void k_lane_estimate(const LaneEstArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ float s_w[SQ_MAX_K];        // a_k, e_k, then w_k
  __shared__ SqBox s_stage[SQ_MAX_K];    // the boxes matched to the current best-row object
  __shared__ unsigned char s_match[SQ_MAX_K * SQ_MAXN];
  __shared__ unsigned char s_n[SQ_MAX_K];
  __shared__ SqBox s_bbox[SQ_MAXN];      // the best row's boxes
  __shared__ int s_bp[SQ_MAXN];          // ... and which of its slots are present
  __shared__ float s_cp[SQ_MAXN + 1];
  __shared__ SqLaneStats s_st;
  const SqairLaneEstimate& o = a.est;
  const LaneRows& v = a.rows;
  const int b = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, K = a.K, N = a.N, R = a.B * K, r = b * K + tid;
  const bool lead = blockIdx.z == 0;
  const size_t tb = (size_t)t * a.B + b, row0 = (size_t)t * R + (size_t)b * K;   // (frame t, particle 0 of lane b)
  const float nan = __builtin_nanf("");
  // ---- 1, 2: weights and the best row
  sq_lane_weights<false>(tid < K ? sq_lane_log_weight<true>(o.log_w, a.lw, t + 1, R, r) : 0.0f, K, s_w, s_st);
  const bool bad = s_st.best < 0;
  if (lead) {
    if (tid == 0) {
      if (o.ess) o.ess[tb] = sq_lane_ess(s_st.S, s_st.Q);
      o.best_row[tb] = bad ? -1 : b * K + s_st.best;
    }
    if (tid < K && o.weights) o.weights[tb * K + tid] = s_w[tid];
    // ---- 4: the best row's slots -> the lane's objects and their boxes
    const size_t best = row0 + (bad ? 0 : s_st.best);
    sq_lane_best_objects(v, best, bad, N, a.H, a.W, tb * N, SqBestOut{o.presence, o.obj_id, o.where, o.box}, s_bp, s_bbox);
    if (o.what)
      for (int i = tid; i < N * a.nw; i += 256) {
        const int j = i / a.nw, q = i - j * a.nw;
        sq_put(o.what + tb * N * a.nw + i, s_bp[j] ? sq_word(a.what + (best * N + j) * a.what_ld + q) : 0u);
      }
    // ---- 3, 5: thread k's particle: its count, and per best-row object its first present slot of maximal IoU
    if (tid < K)
      s_n[tid] = (unsigned char)sq_lane_associate<false>(v, row0 + tid, N, a.H, a.W, o.iou_min, s_bp, s_bbox, s_match + tid * N,
                                                         nullptr, nullptr);
    __syncthreads();
    // ---- 3: the count posterior (thread c), the expected count (thread N + 1), the first maximal count (thread 0)
    if (tid <= N) {
      float p = 0.0f;
      for (int k = 0; k < K; ++k) p += s_n[k] == tid ? s_w[k] : 0.0f;
      if (bad) p = nan;
      s_cp[tid] = p;
      if (o.count_prob) o.count_prob[tb * (N + 1) + tid] = p;
    } else if (tid == N + 1 && o.expected_count) {
      float cnt = 0.0f;
      for (int k = 0; k < K; ++k) cnt += s_w[k] * (float)s_n[k];
      o.expected_count[tb] = cnt;
    }
    __syncthreads();
    if (tid == 0 && o.map_count) {
      int best_c = 0;
      for (int c = 1; c <= N; ++c)
        if (s_cp[c] > s_cp[best_c]) best_c = c;
      o.map_count[tb] = bad ? -1 : best_c;
    }
    // ---- 5: support and consensus box of every best-row object (the loop and its branches are uniform over the workgroup)
    if (o.support || o.box_mean) {
      for (int j = 0; j < N; ++j) {
        const size_t e = tb * N + j;
        if (!s_bp[j]) {   // absent: zero (a non-finite lane: NaN)
          const float z = bad ? nan : 0.0f;
          if (tid == 0 && o.support) o.support[e] = z;
          if (tid < 4 && o.box_mean) o.box_mean[e * 4 + tid] = z;
          continue;
        }
        const int mt = tid < K ? s_match[tid * N + j] : 255;
        if (mt != 255) s_stage[tid] = sq_box_of_where(v.where + (sq_lane_slot(v, row0 + tid, N) + mt) * v.where_ld, a.H, a.W);
        __syncthreads();
        if (tid < 4) {
          float sup, sum;
          sq_lane_box_sum(s_w, s_stage, K, 1, tid, [&](int k) { return s_match[k * N + j] != 255; }, sup, sum);
          if (tid == 0 && o.support) o.support[e] = sup;
          if (o.box_mean) o.box_mean[e * 4 + tid] = sum / sup;
        }
        __syncthreads();
      }
    }
  }
  // ---- 6: the posterior mean reconstruction, this workgroup's chunk of pixels
  if (CANVAS) {
    const int P = a.H * a.W, p0 = blockIdx.z * SQ_EST_PIXELS;
    for (int p = p0 + tid; p < min(p0 + SQ_EST_PIXELS, P); p += 256)
      o.mean_canvas[tb * P + p] = sq_lane_mean_pixel(s_w, a.canvas, row0, P, p, K);
  }
}
int sq_launch_lane_estimate(const LaneEstArgs& a, hipStream_t s) {
  const int P = a.H * a.W, nz = a.est.mean_canvas ? (P + SQ_EST_PIXELS - 1) / SQ_EST_PIXELS : 1;
  if (a.est.mean_canvas) SQ_LAUNCH(k_lane_estimate<true>, dim3(a.B, a.T, nz), dim3(256), 0, s, a);
  else SQ_LAUNCH(k_lane_estimate<false>, dim3(a.B, a.T, nz), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Object layers (sqair_set_layers; LaneLayerArgs in sqair_glue.h; the semantics: include/sqair_hip.h, points 1-7)
// ------------------------------------------------------------------------------------------------
// k_lane_layers: workgroup (lane b, frame t, tile z of SQ_LAYER_TILE consecutive pixels), thread = SQ_LAYER_PX pixels of the tile,
// 256 apart, whose sums it keeps in registers.  Every workgroup repeats the estimate's prologue -- weights, best objects, thread k's
// association into the K x N byte table -- and turns the table into one 64-bit mask per (object, wave): the particles that agree on
// an object are then the set bits, walked in index order by every thread alike.  The matched glimpses pass through two LDS buffers:
// while the taps of pair (j, k) read one, the LDS-DMA of the next pair's G^2 floats and threads 0..4's transform coefficients and
// presence of it fill the other; one barrier per pair.  A pair whose box misses the tile's rows (or the frame's columns) is skipped
// by a test on the box ends that is uniform over the workgroup -- the coordinate grows with the pixel index, and a pixel outside the
// box adds exactly 0 either way.  Nothing is accumulated with atomics.
struct SqLayerPairs { int j, wv; unsigned long long m; };   // the walk's position: object, wave word, bits left in it
__device__ __forceinline__ bool sq_layer_next(const unsigned long long (*s_agree)[4], const int N, SqLayerPairs& it, int& k) {
  for (;;) {
    if (it.m) {
      k = 64 * it.wv + __ffsll(it.m) - 1;
      it.m &= it.m - 1;
      return true;
    }
    if (++it.wv == 4) {
      it.wv = 0;
      if (++it.j >= N) return false;
    }
    it.m = s_agree[it.j][it.wv];
  }
}
__global__ __launch_bounds__(256) void k_lane_layers(const LaneLayerArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  extern __shared__ __align__(16) float s_gl[];   // [2][G * G]: the glimpse of the pair at work, and of the next one
  __shared__ float s_w[SQ_MAX_K];                 // a_k, e_k, then w_k
  __shared__ unsigned char s_match[SQ_MAX_K * SQ_MAXN];
  __shared__ unsigned long long s_agree[SQ_MAXN][4];
  __shared__ SqBox s_bbox[SQ_MAXN];
  __shared__ int s_bp[SQ_MAXN];
  __shared__ float s_co[2][8];                    // sx, sy, tx, ty, presence of the two staged pairs
  __shared__ SqLaneStats s_st;
  constexpr int PX = SQ_LAYER_PX;
  const SqairLaneLayers& o = a.lay;
  const LaneRows& v = a.rows;
  const int b = blockIdx.x, t = blockIdx.y, tid = threadIdx.x, K = a.K, N = a.N, G = a.G, H = a.H, W = a.W, R = a.B * K;
  const int G2 = G * G, P = H * W;
  const size_t tb = (size_t)t * a.B + b, row0 = (size_t)t * R + (size_t)b * K;   // (frame t, particle 0 of lane b)
  const float nan = __builtin_nanf("");
  // ---- the estimate's points 1, 2, 4, 5: weights, best row, its objects, thread k's association
  sq_lane_weights<false>(tid < K ? sq_lane_log_weight<true>(a.log_w, a.lw, t + 1, R, b * K + tid) : 0.0f, K, s_w, s_st);
  const bool bad = s_st.best < 0;
  sq_lane_best_objects(v, row0 + (bad ? 0 : s_st.best), bad, N, H, W, 0, SqBestOut{nullptr, nullptr, nullptr, nullptr}, s_bp, s_bbox);
  if (tid < K) sq_lane_associate<false>(v, row0 + tid, N, H, W, a.iou_min, s_bp, s_bbox, s_match + tid * N, nullptr, nullptr);
  __syncthreads();
  if (blockIdx.z == 0 && o.match)
    for (int i = tid; i < K * N; i += 256) o.match[tb * K * N + i] = s_match[i] == 255 ? -1 : (int)s_match[i];
  if (!o.layer && !o.cover && !o.owner) return;
  for (int j = 0; j < N; ++j) {   // (an absent object, and every object of a non-finite lane: no bit)
    const unsigned long long m = __ballot(tid < K && s_match[tid * N + j] != 255);
    if ((tid & 63) == 0) s_agree[j][tid >> 6] = m;
  }
  // ---- this thread's pixels, the tile's rows
  const int p0 = blockIdx.z * SQ_LAYER_TILE, ya = p0 / W, yb = (min(p0 + SQ_LAYER_TILE, P) - 1) / W;
  int px[PX], py[PX], own[PX];
  float top[PX];
#pragma unroll
  for (int u = 0; u < PX; ++u) {
    const int p = min(p0 + tid + 256 * u, P - 1);   // (clamped: a pixel beyond the frame is computed and not written)
    py[u] = p / W;
    px[u] = p - py[u] * W;
    own[u] = -1;
    top[u] = -__builtin_inff();
  }
  // pair (j, k) into buffer `buf`: the glimpse by LDS-DMA, its coefficients and presence by threads 0..4 -- all in place by the next barrier
  auto stage = [&](const int j, const int k, const int buf) {
    const int m = s_match[k * N + j];
    const size_t sl = sq_lane_slot(v, row0 + k, N) + m;
    sq_wave_stage(s_gl + buf * G2, a.glimpse + ((row0 + k) * N + m) * G2, G2, tid & 63, tid >> 6, 4);
    if (tid < 4) s_co[buf][tid] = sq_to_coord(v.where[sl * v.where_ld + tid], tid);
    else if (tid == 4) s_co[buf][4] = v.presence[sl * v.pres_ld];
  };
  __syncthreads();
  SqLayerPairs it = {-1, 3, 0ull};
  int nk = 0, cur = 0;
  bool more = sq_layer_next(s_agree, N, it, nk);
  int nj = it.j;
  if (more) stage(nj, nk, 0);
  __syncthreads();
  for (int j = 0; j < N; ++j) {   // (the loops and their branches are uniform over the workgroup)
    float lay[PX], cov[PX];
    if (!s_bp[j]) {   // absent: zero (a non-finite lane: NaN)
#pragma unroll
      for (int u = 0; u < PX; ++u) lay[u] = cov[u] = bad ? nan : 0.0f;
    } else {
#pragma unroll
      for (int u = 0; u < PX; ++u) lay[u] = cov[u] = 0.0f;
      float sup = 0.0f;
      while (more && nj == j) {
        const int k = nk;
        more = sq_layer_next(s_agree, N, it, nk);
        nj = it.j;
        if (more) stage(nj, nk, cur ^ 1);
        const float* gk = s_gl + cur * G2;
        const float sx = s_co[cur][0], sy = s_co[cur][1], tx = s_co[cur][2], ty = s_co[cur][3], pk = s_co[cur][4], wk = s_w[k];
        sup += wk;
        const bool hit = sq_canvas_coord(yb, H, sy, ty, G) > -1.0f && sq_canvas_coord(ya, H, sy, ty, G) < (float)G &&
                         sq_canvas_coord(W - 1, W, sx, tx, G) > -1.0f && sq_canvas_coord(0, W, sx, tx, G) < (float)G;
        if (hit) {
#pragma unroll
          for (int u = 0; u < PX; ++u) {
            const float xg = sq_canvas_coord(px[u], W, sx, tx, G), yg = sq_canvas_coord(py[u], H, sy, ty, G);
            if (sq_canvas_inside(xg, G) && sq_canvas_inside(yg, G)) {
              float val, on;
              sq_canvas_tap(gk, xg, yg, G, val, on);
              lay[u] += wk * (val * pk);
              cov[u] += wk * (on * pk);
            }
          }
        }
        __syncthreads();
        cur ^= 1;
      }
#pragma unroll
      for (int u = 0; u < PX; ++u) {
        lay[u] /= sup;
        cov[u] /= sup;
        if (cov[u] > top[u]) { top[u] = cov[u]; own[u] = j; }   // (the first of equal covers stays; a NaN never wins)
      }
    }
#pragma unroll
    for (int u = 0; u < PX; ++u) {
      const int p = p0 + tid + 256 * u;
      if (p >= P) continue;
      if (o.layer) o.layer[(tb * N + j) * P + p] = lay[u];
      if (o.cover) o.cover[(tb * N + j) * P + p] = cov[u];
    }
  }
  if (o.owner) {
#pragma unroll
    for (int u = 0; u < PX; ++u) {
      const int p = p0 + tid + 256 * u;
      if (p < P) o.owner[tb * P + p] = top[u] >= o.cover_min ? own[u] : -1;
    }
  }
}
int sq_launch_lane_layers(const LaneLayerArgs& a, hipStream_t s) {
  const int P = a.H * a.W, lds = 2 * a.G * a.G * (int)sizeof(float);
  const int nz = (a.lay.layer || a.lay.cover || a.lay.owner) ? (P + SQ_LAYER_TILE - 1) / SQ_LAYER_TILE : 1;
  if (lds > 32 * 1024 && sq_allow_big_lds((const void*)k_lane_layers, 150 * 1024) != 0) return -2;
  SQ_LAUNCH(k_lane_layers, dim3(a.B, a.T, nz), dim3(256), lds, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Stream scoring (sqair_set_score; LaneScoreArgs in sqair_glue.h; the semantics: include/sqair_hip.h, points 0-6)
// ------------------------------------------------------------------------------------------------
// k_lane_score: workgroup = lane b, looping over the pass's frames in order -- the identity memory makes frame t depend on frame
// t - 1.  Per frame thread i < G * N fills entry (g, j) = (i / N, i % N) of the IoU table in LDS (-1 for a pair that is no
// candidate), thread 0 walks the tables (sq_assign_keep_greedy) and counts the events, threads g < G write the per-frame outputs.
// The memory stays in LDS over the frames; thread 0 keeps the counters in registers and adds them to the accumulators once, in
// place.  Every branch around a barrier depends on truth_valid[t, b] and map_count[t, b] alone: uniform over the workgroup.
// OPT (sqair_set_lane_match, score = 1): wave 0 makes the assignment (sq_assign_keep_optimal, its int32 table in LDS) where thread 0
// walks the greedy one; everything after it is the same code reading s_gm / s_claim.  OPT = false is k_lane_score as it always was.
template <bool OPT>
__device__ __forceinline__ void sq_lane_score_frames(const LaneScoreArgs& a) {
  __shared__ float s_iou[SQ_SCORE_MAXG * SQ_MAXN];
  __shared__ int s_last[SQ_SCORE_MAXG], s_tpres[SQ_SCORE_MAXG], s_gm[SQ_SCORE_MAXG];
  __shared__ int s_id[SQ_MAXN], s_lpres[SQ_MAXN], s_claim[SQ_MAXN];
  const SqairLaneScore& o = a.sc;
  const int b = blockIdx.x, tid = threadIdx.x, G = o.G, N = a.N;
  if (tid < G) s_last[tid] = o.last_id[(size_t)b * G + tid];
  long long c_frames = 0, c_invalid = 0, c_truth = 0, c_tp = 0, c_fn = 0, c_fp = 0, c_idsw = 0, c_hit = 0, c_err = 0;
  double iou_sum = tid == 0 ? o.iou_sum[b] : 0.0;
  for (int t = 0; t < a.T; ++t) {
    const size_t tb = (size_t)t * a.B + b;
    const bool valid = o.truth_valid[tb] != 0;
    const int mc = a.map_count[tb];
    __syncthreads();   // (the memory is loaded; the last frame's readers are done with the tables)
    if (!valid || mc == -1) {   // no truth, or a non-finite lane: nothing is scored
      if (tid == 0) {
        if (valid) ++c_invalid;
        if (o.tp) o.tp[tb] = -1;
        if (o.fn) o.fn[tb] = -1;
        if (o.fp) o.fp[tb] = -1;
        if (o.idsw) o.idsw[tb] = -1;
      }
      if (tid < G) {
        if (o.truth_match) o.truth_match[tb * G + tid] = -1;
        if (o.match_iou) o.match_iou[tb * G + tid] = 0.0f;
      }
      continue;
    }
    // ---- 1: the candidates' IoU
    if (tid < G * N) {
      const int g = tid / N, j = tid - g * N;
      float v = -1.0f;
      if (o.truth_present[tb * G + g] != 0 && a.presence[tb * N + j] != 0.0f) {
        const float* p = o.truth_box + (tb * G + g) * 4;
        const float* q = a.box + (tb * N + j) * 4;
        v = sq_box_iou(SqBox{p[0], p[1], p[2], p[3]}, SqBox{q[0], q[1], q[2], q[3]});
      }
      s_iou[tid] = v;
    }
    if (tid < G) s_tpres[tid] = o.truth_present[tb * G + tid] != 0;
    if (tid < N) {
      s_lpres[tid] = a.presence[tb * N + tid] != 0.0f;
      s_id[tid] = (int)sq_word(a.obj_id + tb * N + tid);
    }
    __syncthreads();
    // ---- 2, 3, 4: the assignment and the events, one thread
    if constexpr (OPT) {
      __shared__ int s_w[SQ_SCORE_MAXG * SQ_MAXN];
      if (tid < 64) sq_assign_keep_optimal(s_iou, N, G, N, o.iou_min, s_last, s_id, s_gm, s_claim, s_w);
    }
    if (tid == 0) {
      if constexpr (!OPT) sq_assign_keep_greedy(s_iou, N, G, N, o.iou_min, s_last, s_id, s_gm, s_claim);
      int n_truth = 0, tp = 0, fn = 0, fp = 0, sw = 0;
      for (int g = 0; g < G; ++g) {
        if (!s_tpres[g]) continue;
        ++n_truth;
        const int j = s_gm[g];
        if (j < 0) { ++fn; continue; }
        ++tp;
        const int id = s_id[j], last = s_last[g];
        sw += last >= 0 && last != id;
        s_last[g] = id;
        iou_sum += (double)s_iou[g * N + j];
      }
      for (int j = 0; j < N; ++j) fp += s_lpres[j] && !s_claim[j];
      ++c_frames; c_truth += n_truth; c_tp += tp; c_fn += fn; c_fp += fp; c_idsw += sw;
      c_hit += mc == n_truth; c_err += mc > n_truth ? mc - n_truth : n_truth - mc;
      if (o.tp) o.tp[tb] = tp;
      if (o.fn) o.fn[tb] = fn;
      if (o.fp) o.fp[tb] = fp;
      if (o.idsw) o.idsw[tb] = sw;
    }
    __syncthreads();
    if (tid < G) {
      const int j = s_gm[tid];
      if (o.truth_match) o.truth_match[tb * G + tid] = j;
      if (o.match_iou) o.match_iou[tb * G + tid] = j >= 0 ? s_iou[tid * N + j] : 0.0f;
    }
  }
  __syncthreads();
  if (tid < G) o.last_id[(size_t)b * G + tid] = s_last[tid];
  if (tid == 0) {
    int64_t* c = o.counts + (size_t)b * SQAIR_SCORE_COUNTS;
    c[0] += c_frames; c[1] += c_invalid; c[2] += c_truth; c[3] += c_tp; c[4] += c_fn; c[5] += c_fp; c[6] += c_idsw; c[7] += c_hit;
    c[8] += c_err;
    o.iou_sum[b] = iou_sum;
  }
}
__global__ __launch_bounds__(256) void k_lane_score(const LaneScoreArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_score_frames<false>(a);
}
__global__ __launch_bounds__(256) void k_lane_score_opt(const LaneScoreArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_score_frames<true>(a);
}
int sq_launch_lane_score(const LaneScoreArgs& a, hipStream_t s) {
  if (a.match) SQ_LAUNCH(k_lane_score_opt, dim3(a.B), dim3(256), 0, s, a);
  else SQ_LAUNCH(k_lane_score, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Lane identities (sqair_set_identity; LaneIdentArgs in sqair_glue.h; the semantics: include/sqair_hip.h, points 0-9)
// ------------------------------------------------------------------------------------------------
// k_lane_identity: workgroup = lane b, looping over the pass's frames in order -- the track table makes frame t depend on frame
// t - 1 -- with the table (ids, words, ages, lengths, boxes, what vectors) in LDS across them.  Per frame thread i < M * N fills entry
// (e, j) = (i / N, i % N) of the IoU table (-1 for a pair that is no candidate) and, when re-identification is on, of the dc2 and dw
// tables: the loop over n_what per pair is the parallel part.  Thread 0 walks the tables -- sq_assign_keep_greedy, then the
// re-identification, the births and the ageing -- and leaves per slot j its entry and how it got there; then threads j < N write
// the outputs and the workgroup copies the words of every seen slot into its entry.  Every array is in LDS, nothing is indexed in
// registers.  Every branch around a barrier depends on best_row[t, b] and the struct's scalars alone: uniform over the workgroup.
// OPT (sqair_set_lane_match, identity = 1): wave 0 makes step 2's assignment (sq_assign_keep_optimal) where thread 0 walks the
// greedy one; the re-identification, the births and the ageing are thread 0's walk either way.  OPT = false is k_lane_identity as
// it always was.
// MOTION (sqair_set_motion; the motion paragraph of include/sqair_hip.h, points P and U): a constant-velocity filter per entry and
// axis of the box centre, its five words (p, v, Ppp, Ppv, Pvv) in LDS with the rest of the table.  Threads i < 2M predict before step 1
// (one barrier more, under the same uniform condition), step 1 reads the predicted box, s_dc2 holds d2 where it holds dc2, step 4's gate is
// d2 <= gate * gate, and threads i < 2N update (or start) the filter of the entry their slot took and write velocity and nis.
// MOTION = false is the code above, statement for statement.
template <bool OPT, bool MOTION>
__device__ __forceinline__ void sq_lane_identity_frames(const LaneIdentArgs& a) {
  __shared__ float s_iou[SQ_IDENT_MAXM * SQ_MAXN], s_dc2[SQ_IDENT_MAXM * SQ_MAXN], s_dw[SQ_IDENT_MAXM * SQ_MAXN];
  __shared__ float s_tbox[SQ_IDENT_MAXM * 4], s_twhat[SQ_IDENT_MAXM * SQ_MAX_NWHAT];
  __shared__ int s_tid[SQ_IDENT_MAXM], s_word[SQ_IDENT_MAXM], s_age[SQ_IDENT_MAXM], s_len[SQ_IDENT_MAXM];
  __shared__ int s_keep[SQ_IDENT_MAXM], s_em[SQ_IDENT_MAXM];                       // keep_id of the walk; the slot an entry took
  __shared__ int s_jid[SQ_MAXN], s_pres[SQ_MAXN], s_claim[SQ_MAXN], s_je[SQ_MAXN], s_how[SQ_MAXN];   // per slot: word, present, entry, how
  const SqairLaneIdentity& o = a.id;
  const int b = blockIdx.x, tid = threadIdx.x, M = o.M, N = a.N, nw = a.nw;
  const bool reid = o.reid_dist > 0.0f, app = o.trk_what != nullptr;
  __shared__ float s_kf[MOTION ? SQ_IDENT_MAXM * 2 * 5 : 1], s_S[MOTION ? SQ_IDENT_MAXM * 2 : 1];   // (p, v, Ppp, Ppv, Pvv) and S per (entry, axis)
  const SqairLaneMotion& mo = a.mo;
  if constexpr (MOTION)
    if (tid < M * 10) s_kf[tid] = mo.trk_kf[(size_t)b * M * 10 + tid];
  if (tid < M) {
    const size_t e = (size_t)b * M + tid;
    s_tid[tid] = o.trk_id[e]; s_word[tid] = o.trk_word[e]; s_age[tid] = o.trk_age[e]; s_len[tid] = o.trk_len[e];
  }
  if (tid < M * 4) s_tbox[tid] = o.trk_box[(size_t)b * M * 4 + tid];
  if (app)
    for (int i = tid; i < M * nw; i += 256) s_twhat[i] = o.trk_what[(size_t)b * M * nw + i];
  int next = tid == 0 ? o.next_id[b] : 0;
  long long c_frames = 0, c_invalid = 0, c_obj = 0, c_kept = 0, c_bridged = 0, c_reid = 0, c_born = 0, c_ended = 0;
  for (int t = 0; t < a.T; ++t) {
    const size_t tb = (size_t)t * a.B + b;
    const bool bad = a.best_row[tb] == -1;
    __syncthreads();   // (the memory is loaded, or the last frame's words are in it; its readers are done with the tables)
    if (bad) {   // a non-finite lane: no outputs, no ageing
      if (tid == 0) ++c_invalid;
      if (tid < N) {
        o.lane_id[tb * N + tid] = -1;
        if (o.how) o.how[tb * N + tid] = -1;
        if (o.track_len) o.track_len[tb * N + tid] = -1;
      }
      if constexpr (MOTION) {
        if (tid < N * 2) mo.velocity[tb * N * 2 + tid] = 0.0f;
        if (tid < N && mo.nis) mo.nis[tb * N + tid] = 0.0f;
      }
      continue;
    }
    // ---- P: every live entry's filter one frame on, per (entry, axis)
    if constexpr (MOTION) {
      if (tid < M * 2 && s_tid[tid >> 1] >= 0) {
        s_S[tid] = sq_kf_predict(s_kf + tid * 5, mo.q, mo.r);
      }
      __syncthreads();
    }
    // ---- 1 (and 4's tables): entry e against slot j
    if (tid < M * N) {
      const int e = tid / N, j = tid - e * N;
      float v = -1.0f, dc2 = 0.0f, dw = 0.0f;
      if (s_tid[e] >= 0 && a.presence[tb * N + j] != 0.0f) {
        const float* q = a.box + (tb * N + j) * 4;
        SqBox p = {s_tbox[e * 4 + 0], s_tbox[e * 4 + 1], s_tbox[e * 4 + 2], s_tbox[e * 4 + 3]};
        const SqBox bx = {q[0], q[1], q[2], q[3]};
        if constexpr (MOTION) {   // the predicted box: the filter's centre, the last seen size
          p.y = s_kf[e * 10] - 0.5f * p.h;
          p.x = s_kf[e * 10 + 5] - 0.5f * p.w;
        }
        v = sq_box_iou(p, bx);
        if constexpr (MOTION) {
          const float dy = fmaf(0.5f, bx.h, bx.y) - s_kf[e * 10], dx = fmaf(0.5f, bx.w, bx.x) - s_kf[e * 10 + 5];
          dc2 = (dy * dy) / s_S[e * 2] + (dx * dx) / s_S[e * 2 + 1];
        }
        if (reid) {
          if constexpr (!MOTION) {
            const float dy = fmaf(0.5f, bx.h, bx.y) - fmaf(0.5f, p.h, p.y), dx = fmaf(0.5f, bx.w, bx.x) - fmaf(0.5f, p.w, p.x);
            dc2 = fmaf(dy, dy, dx * dx);
          }
          if (app) {
            const float* wj = a.what + (tb * N + j) * nw;
            float acc = 0.0f;
            for (int c = 0; c < nw; ++c) {
              const float d = wj[c] - s_twhat[e * nw + c];
              acc = fmaf(d, d, acc);
            }
            dw = acc / (float)nw;
          }
        }
      }
      s_iou[tid] = v; s_dc2[tid] = dc2; s_dw[tid] = dw;
    }
    if (tid < M) s_keep[tid] = s_tid[tid] >= 0 ? s_word[tid] : -1;
    if (tid < N) {
      s_pres[tid] = a.presence[tb * N + tid] != 0.0f;
      s_jid[tid] = (int)sq_word(a.obj_id + tb * N + tid);
    }
    __syncthreads();
    // ---- 2 .. 8: the links, the births and the ageing, one thread
    if constexpr (OPT) {
      __shared__ int s_w[SQ_IDENT_MAXM * SQ_MAXN];
      if (tid < 64) sq_assign_keep_optimal(s_iou, N, M, N, o.iou_min, s_keep, s_jid, s_em, s_claim, s_w);
    }
    if (tid == 0) {
      if constexpr (!OPT) sq_assign_keep_greedy(s_iou, N, M, N, o.iou_min, s_keep, s_jid, s_em, s_claim);
      for (int j = 0; j < N; ++j) { s_je[j] = -1; s_how[j] = -1; }
      for (int e = 0; e < M; ++e) {
        const int j = s_em[e];
        if (j < 0) continue;
        s_je[j] = e;
        s_how[j] = s_word[e] == s_jid[j] ? 1 : 2;
      }
      if (reid)
        for (int j = 0; j < N; ++j) {
          if (!s_pres[j] || s_je[j] >= 0) continue;
          int be = -1;
          float bk = 0.0f;
          for (int e = 0; e < M; ++e) {
            if (s_tid[e] < 0 || s_em[e] >= 0) continue;
            if constexpr (MOTION) {
              if (!(s_dc2[e * N + j] <= mo.gate * mo.gate)) continue;
            } else {
              const float r = o.reid_dist * (float)(s_age[e] + 1);
              if (!(s_dc2[e * N + j] <= r * r)) continue;
            }
            if (app && !(s_dw[e * N + j] <= o.reid_what)) continue;
            const float key = app ? s_dw[e * N + j] : s_dc2[e * N + j];
            if (be < 0 || key < bk) { be = e; bk = key; }
          }
          if (be < 0) continue;
          s_em[be] = j; s_je[j] = be; s_how[j] = 3;
        }
      for (int j = 0; j < N; ++j) {   // 5: the matched entries
        const int e = s_je[j];
        if (e < 0) continue;
        s_word[e] = s_jid[j]; s_age[e] = 0; s_len[e] += 1;
      }
      for (int j = 0; j < N; ++j) {   // 6: births
        if (!s_pres[j] || s_je[j] >= 0) continue;
        int be = -1;
        for (int e = 0; e < M && be < 0; ++e)
          if (s_tid[e] < 0) be = e;
        if (be < 0) {
          for (int e = 0; e < M; ++e)
            if (s_em[e] < 0 && (be < 0 || s_age[e] > s_age[be])) be = e;
          ++c_ended;
        }
        s_tid[be] = next++; s_word[be] = s_jid[j]; s_age[be] = 0; s_len[be] = 1;
        s_em[be] = j; s_je[j] = be; s_how[j] = 0;
      }
      for (int e = 0; e < M; ++e) {   // 7: ageing
        if (s_tid[e] < 0 || s_em[e] >= 0) continue;
        s_age[e] += 1;
        if (s_age[e] > o.max_age) { s_tid[e] = -1; ++c_ended; }
      }
      ++c_frames;
      for (int j = 0; j < N; ++j) {
        const int hw = s_how[j];
        c_obj += s_pres[j]; c_born += hw == 0; c_kept += hw == 1; c_bridged += hw == 2; c_reid += hw == 3;
      }
    }
    __syncthreads();
    // ---- 5, 6: the outputs, and the words of every seen slot into its entry
    if (tid < N) {
      const int e = s_je[tid];
      o.lane_id[tb * N + tid] = e >= 0 ? s_tid[e] : -1;
      if (o.how) o.how[tb * N + tid] = s_how[tid];
      if (o.track_len) o.track_len[tb * N + tid] = e >= 0 ? s_len[e] : -1;
    }
    // ---- U: the filter of every entry a slot took, per (slot, axis): the update of a linked one, the start of a born one
    if constexpr (MOTION) {
      if (tid < N * 2) {
        const int j = tid >> 1, ax = tid & 1, e = s_je[j];
        float vel = 0.0f, nis = 0.0f;
        if (e >= 0) {
          const float* q = a.box + (tb * N + j) * 4;
          const float z = fmaf(0.5f, q[2 + ax], q[ax]);
          float* k = s_kf + (e * 2 + ax) * 5;
          if (s_how[j] == 0) {
            k[0] = z; k[1] = 0.0f; k[2] = mo.r; k[3] = 0.0f; k[4] = mo.v0_var;
          } else {
            const float S = s_S[e * 2 + ax], ppp = k[2], ppv = k[3];
            const float y = z - k[0], k0 = ppp / S, k1 = ppv / S;
            k[0] = fmaf(k0, y, k[0]);
            vel = fmaf(k1, y, k[1]);
            k[1] = vel;
            k[2] = (1.0f - k0) * ppp;
            k[3] = (1.0f - k0) * ppv;
            k[4] = fmaf(-k1, ppv, k[4]);
            nis = s_dc2[e * N + j];
          }
        }
        mo.velocity[tb * N * 2 + tid] = vel;
        if (ax == 0 && mo.nis) mo.nis[tb * N + j] = nis;
      }
    }
    if (tid < N * 4) {
      const int j = tid >> 2, e = s_je[j];
      if (e >= 0) sq_put(s_tbox + e * 4 + (tid & 3), sq_word(a.box + (tb * N + j) * 4 + (tid & 3)));
    }
    if (app)
      for (int i = tid; i < N * nw; i += 256) {
        const int j = i / nw, e = s_je[j];
        if (e >= 0) sq_put(s_twhat + e * nw + (i - j * nw), sq_word(a.what + tb * N * nw + i));
      }
  }
  __syncthreads();
  if (tid < M) {
    const size_t e = (size_t)b * M + tid;
    o.trk_id[e] = s_tid[tid]; o.trk_word[e] = s_word[tid]; o.trk_age[e] = s_age[tid]; o.trk_len[e] = s_len[tid];
  }
  if (tid < M * 4) sq_put(o.trk_box + (size_t)b * M * 4 + tid, sq_word(s_tbox + tid));
  if (app)
    for (int i = tid; i < M * nw; i += 256) sq_put(o.trk_what + (size_t)b * M * nw + i, sq_word(s_twhat + i));
  if constexpr (MOTION)
    if (tid < M * 10) sq_put(mo.trk_kf + (size_t)b * M * 10 + tid, sq_word(s_kf + tid));
  if (tid == 0) {
    o.next_id[b] = next;
    int64_t* c = o.counts + (size_t)b * SQAIR_IDENT_COUNTS;
    c[0] += c_frames; c[1] += c_invalid; c[2] += c_obj; c[3] += c_kept; c[4] += c_bridged; c[5] += c_reid; c[6] += c_born; c[7] += c_ended;
  }
}
__global__ __launch_bounds__(256) void k_lane_identity(const LaneIdentArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_identity_frames<false, false>(a);
}
__global__ __launch_bounds__(256) void k_lane_identity_opt(const LaneIdentArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_identity_frames<true, false>(a);
}
__global__ __launch_bounds__(256) void k_lane_identity_motion(const LaneIdentArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_identity_frames<false, true>(a);
}
__global__ __launch_bounds__(256) void k_lane_identity_motion_opt(const LaneIdentArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_identity_frames<true, true>(a);
}
int sq_launch_lane_identity(const LaneIdentArgs& a, hipStream_t s) {
  if (a.motion && a.match) SQ_LAUNCH(k_lane_identity_motion_opt, dim3(a.B), dim3(256), 0, s, a);
  else if (a.motion) SQ_LAUNCH(k_lane_identity_motion, dim3(a.B), dim3(256), 0, s, a);
  else if (a.match) SQ_LAUNCH(k_lane_identity_opt, dim3(a.B), dim3(256), 0, s, a);
  else SQ_LAUNCH(k_lane_identity, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Trajectory scoring (sqair_lane_traj_score; LaneTrajScoreArgs in sqair_glue.h; the semantics: include/sqair_hip.h, points 0-6)
// ------------------------------------------------------------------------------------------------
// k_lane_traj_score: grid (lane b, chunk z of SQ_TRAJ_FRAMES frames).  Every workgroup recomputes its lane's link -- thread i < G * N
// fills entry (g, j) = (i / N, i % N) of the IoU table in LDS (-1 for a pair that is no candidate; every pair of a lane that is not
// scored), thread 0 walks it (sq_assign_keep_greedy) -- and chunk 0 alone writes lane_counts and the [B, G] outputs.  Then thread =
// frame f = z * SQ_TRAJ_FRAMES + tid, looping over the truth slots with the link read from LDS: it owns the cells (f, b) of counts
// and sums.  The barriers are met by every thread: what differs between lanes is what the threads store around them.
// OPT (sqair_set_lane_match, traj_link = 1): wave 0 makes the link (sq_assign_keep_optimal) where thread 0 walks the greedy one.
// OPT = false is k_lane_traj_score as it always was.
template <bool OPT>
__device__ __forceinline__ void sq_lane_traj_score_frames(const LaneTrajScoreArgs& a) {
  __shared__ float s_iou[SQ_SCORE_MAXG * SQ_MAXN];
  __shared__ int s_keep[SQ_SCORE_MAXG], s_gm[SQ_SCORE_MAXG], s_apres[SQ_SCORE_MAXG];
  __shared__ int s_id[SQ_MAXN], s_claim[SQ_MAXN];
  const SqairLaneTraj& t = a.tab;
  const SqairTrajTruth& u = a.tr;
  const SqairTrajScore& o = a.sc;
  const int b = blockIdx.x, tid = threadIdx.x, G = u.G, N = a.N;
  const bool anchored = u.anchor_valid[b] != 0;
  const bool lane_on = anchored && t.best_row[b] != -1;   // (a non-finite lane has no objects to link)
  // ---- 1: the link
  if (tid < G * N) {
    const int g = tid / N, j = tid - g * N;
    float v = -1.0f;
    if (lane_on && u.anchor_present[(size_t)b * G + g] != 0 && t.presence[(size_t)b * N + j] != 0.0f) {
      const float* p = u.anchor_box + ((size_t)b * G + g) * 4;
      const float* q = t.box0 + ((size_t)b * N + j) * 4;
      v = sq_box_iou(SqBox{p[0], p[1], p[2], p[3]}, SqBox{q[0], q[1], q[2], q[3]});
    }
    s_iou[tid] = v;
  }
  if (tid < G) {
    s_apres[tid] = lane_on && u.anchor_present[(size_t)b * G + tid] != 0;
    s_keep[tid] = u.keep_id ? u.keep_id[(size_t)b * G + tid] : -1;
  }
  if (tid < N) s_id[tid] = t.obj_id ? (int)sq_word(t.obj_id + (size_t)b * N + tid) : 0;
  __syncthreads();
  if constexpr (OPT) {
    __shared__ int s_w[SQ_SCORE_MAXG * SQ_MAXN];
    if (tid < 64) sq_assign_keep_optimal(s_iou, N, G, N, o.iou_min, u.keep_id ? s_keep : nullptr, s_id, s_gm, s_claim, s_w);
  } else {
    if (tid == 0) sq_assign_keep_greedy(s_iou, N, G, N, o.iou_min, u.keep_id ? s_keep : nullptr, s_id, s_gm, s_claim);
  }
  __syncthreads();
  if (blockIdx.y == 0) {
    if (tid < G) {
      const int j = s_gm[tid];
      if (o.link) o.link[(size_t)b * G + tid] = j;
      if (o.link_iou) o.link_iou[(size_t)b * G + tid] = j >= 0 ? s_iou[tid * N + j] : 0.0f;
    }
    if (tid == 0 && anchored) {
      int64_t* c = o.lane_counts + (size_t)b * SQAIR_TRAJ_LANE_COUNTS;
      if (!lane_on) {
        c[1] += 1;
      } else {
        int n_anchor = 0, n_link = 0;
        for (int g = 0; g < G; ++g) { n_anchor += s_apres[g]; n_link += s_gm[g] >= 0; }
        c[0] += 1; c[2] += n_anchor; c[3] += n_link;
      }
    }
  }
  // ---- 2, 3, 4: one frame per thread
  const int f = blockIdx.y * SQ_TRAJ_FRAMES + tid;
  if (f >= a.F) return;   // (past the last barrier)
  const size_t fb = (size_t)f * a.B + b;
  const bool on = lane_on && u.truth_valid[fb] != 0 && (!t.valid_mass || t.valid_mass[fb] > 0.0f);
  long long c_pairs = 0, c_hits = 0, c_lost = 0, c_gone = 0;
  double* sum = o.sums + fb * SQAIR_TRAJ_SUMS;
  double iou_sum = 0.0, err_sum = 0.0, brier_sum = 0.0;
  if (on) { iou_sum = sum[0]; err_sum = sum[1]; brier_sum = sum[2]; }
  int n_truth = 0;
  for (int g = 0; g < G; ++g) {
    const int j = s_gm[g];
    const bool y = on && u.truth_present[fb * G + g] != 0;
    n_truth += y;
    int st = -1;
    float p = 0.0f, iou = 0.0f, err = 0.0f;
    if (on && j >= 0) {
      const float al = t.alive[fb * N + j];
      p = al / t.support[(size_t)b * N + j];
      const float d = p - (y ? 1.0f : 0.0f);
      brier_sum += (double)(d * d);
      if (!y) {
        st = 0; ++c_gone;
      } else if (al > 0.0f) {
        st = 1; ++c_pairs;
        const float* tb = u.truth_box + (fb * G + g) * 4;
        const float* q = t.box_mean + (fb * N + j) * 4;
        iou = sq_box_iou(SqBox{tb[0], tb[1], tb[2], tb[3]}, SqBox{q[0], q[1], q[2], q[3]});
        const float dy = (tb[0] + 0.5f * tb[2]) - (q[0] + 0.5f * q[2]), dx = (tb[1] + 0.5f * tb[3]) - (q[1] + 0.5f * q[3]);
        err = sqrtf(dy * dy + dx * dx);
        c_hits += iou >= o.iou_min;
        iou_sum += (double)iou; err_sum += (double)err;
      } else {
        st = 2; ++c_lost;   // (box_mean is NaN there: not read)
      }
    }
    if (o.state) o.state[fb * G + g] = st;
    if (o.p_alive) o.p_alive[fb * G + g] = p;
    if (o.pair_iou) o.pair_iou[fb * G + g] = iou;
    if (o.centre_err) o.centre_err[fb * G + g] = err;
  }
  int cm = -1;
  if (on) {
    const float* cp = t.count_prob + fb * (N + 1);
    float top = cp[0];
    cm = 0;
    for (int c = 1; c <= N; ++c)
      if (cp[c] > top) { top = cp[c]; cm = c; }
    int64_t* c = o.counts + fb * SQAIR_TRAJ_COUNTS;
    c[0] += 1; c[1] += c_pairs; c[2] += c_hits; c[3] += c_lost; c[4] += c_gone; c[5] += cm == n_truth;
    c[6] += cm > n_truth ? cm - n_truth : n_truth - cm;
    sum[0] = iou_sum; sum[1] = err_sum; sum[2] = brier_sum;
  }
  if (o.count_map) o.count_map[fb] = cm;
}
__global__ __launch_bounds__(256) void k_lane_traj_score(const LaneTrajScoreArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_traj_score_frames<false>(a);
}
__global__ __launch_bounds__(256) void k_lane_traj_score_opt(const LaneTrajScoreArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  sq_lane_traj_score_frames<true>(a);
}
int sq_launch_lane_traj_score(const LaneTrajScoreArgs& a, hipStream_t s) {
  const dim3 grid(a.B, (a.F + SQ_TRAJ_FRAMES - 1) / SQ_TRAJ_FRAMES);
  if (a.match) SQ_LAUNCH(k_lane_traj_score_opt, grid, dim3(256), 0, s, a);
  else SQ_LAUNCH(k_lane_traj_score, grid, dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// IDF1 scoring (sqair_set_idf; LaneIdfArgs / LaneIdfSolveArgs in sqair_glue.h; the semantics: include/sqair_hip.h, points 1-5)
// ------------------------------------------------------------------------------------------------
// k_lane_idf: workgroup = lane b, looping over the pass's frames in order with the lane's table in LDS across them (a free column
// loads as zeros: its stale words are never read).  Per scored frame thread 0 finds or makes the column of every present lane
// object (at most N * P compares) and counts the column, the unkeyed objects and the frame; threads g < G count their truth's
// presence, match and fragmentation; then thread i < G * N computes the IoU of pair (g, j) = (i / N, i % N) on the words the score
// read and increments its own cell of the overlap table -- the columns of a frame are distinct, so every cell has one writer.
// Everything is in LDS, nothing is indexed in registers.  Every branch around a barrier depends on truth_valid[t, b] and
// map_count[t, b] alone: uniform over the workgroup.
__global__ __launch_bounds__(256) void k_lane_idf(const LaneIdfArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ int s_ov[SQ_SCORE_MAXG * SQ_IDF_MAXP];
  __shared__ int s_cid[SQ_IDF_MAXP], s_cfr[SQ_IDF_MAXP];
  __shared__ int s_rfr[SQ_SCORE_MAXG], s_mat[SQ_SCORE_MAXG], s_frag[SQ_SCORE_MAXG], s_st[SQ_SCORE_MAXG];
  __shared__ int s_jcol[SQ_MAXN];
  const SqairLaneScore& o = a.sc;
  const SqairLaneIdf& f = a.idf;
  const int b = blockIdx.x, tid = threadIdx.x, G = o.G, N = a.N, P = f.P;
  if (tid < P) {
    s_cid[tid] = f.col_id[(size_t)b * P + tid];
    s_cfr[tid] = s_cid[tid] >= 0 ? f.col_frames[(size_t)b * P + tid] : 0;
  }
  if (tid < G) {
    const size_t e = (size_t)b * G + tid;
    s_rfr[tid] = f.row_frames[e]; s_mat[tid] = f.matched[e]; s_frag[tid] = f.frag[e]; s_st[tid] = f.trk_state[e];
  }
  for (int i = tid; i < G * P; i += 256) s_ov[i] = f.col_id[(size_t)b * P + i % P] >= 0 ? f.overlap[(size_t)b * G * P + i] : 0;
  int c_extra = 0, c_frames = 0, c_over = 0;   // (thread 0's)
  for (int t = 0; t < a.T; ++t) {
    const size_t tb = (size_t)t * a.B + b;
    if (o.truth_valid[tb] == 0 || a.map_count[tb] == -1) continue;   // no truth, or a non-finite lane: nothing is touched
    __syncthreads();   // (the table is loaded; the last frame's increments are in it)
    // ---- a, b: the columns of the frame's objects, one thread
    if (tid == 0) {
      int unkeyed = 0;
      for (int j = 0; j < N; ++j) {
        s_jcol[j] = -1;
        if (a.presence[tb * N + j] == 0.0f) continue;
        const int word = (int)sq_word(a.ids + tb * N + j);
        bool fresh;
        const int col = sq_lane_id_column(s_cid, P, word, s_jcol, j, fresh);
        if (fresh) {
          s_cfr[col] = 0;
          for (int g = 0; g < G; ++g) s_ov[g * P + col] = 0;
        }
        if (col >= 0) { s_jcol[j] = col; s_cfr[col] += 1; }
        else ++unkeyed;
      }
      c_extra += unkeyed; c_over += unkeyed > 0; ++c_frames;
    }
    // ---- c, e, f: the truth's counters, thread g
    if (tid < G && o.truth_present[tb * G + tid] != 0) {
      const int m = o.truth_match[tb * G + tid] >= 0, st = s_st[tid];
      s_rfr[tid] += 1; s_mat[tid] += m;
      s_frag[tid] += m && (st & 2) && !(st & 1);
      s_st[tid] = (st & 2) | (m ? 3 : 0);
    }
    __syncthreads();
    // ---- d: every overlapping pair
    if (tid < G * N) {
      const int g = tid / N, j = tid - g * N, col = s_jcol[j];
      if (col >= 0 && o.truth_present[tb * G + g] != 0) {
        const float* p = o.truth_box + (tb * G + g) * 4;
        const float* q = a.box + (tb * N + j) * 4;
        if (sq_box_iou(SqBox{p[0], p[1], p[2], p[3]}, SqBox{q[0], q[1], q[2], q[3]}) >= o.iou_min) s_ov[g * P + col] += 1;
      }
    }
  }
  __syncthreads();
  if (tid < P) { f.col_id[(size_t)b * P + tid] = s_cid[tid]; f.col_frames[(size_t)b * P + tid] = s_cfr[tid]; }
  if (tid < G) {
    const size_t e = (size_t)b * G + tid;
    f.row_frames[e] = s_rfr[tid]; f.matched[e] = s_mat[tid]; f.frag[e] = s_frag[tid]; f.trk_state[e] = s_st[tid];
  }
  for (int i = tid; i < G * P; i += 256) f.overlap[(size_t)b * G * P + i] = s_ov[i];
  if (tid == 0) {
    f.extra_frames[b] += c_extra; f.frames[b] += c_frames;
    f.totals[(size_t)b * SQAIR_IDF_TOTALS + 11] += c_over;
  }
}
int sq_launch_lane_idf(const LaneIdfArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_idf, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// k_lane_idf_solve: workgroup = lane b, ONE wavefront.  The lane's overlap table to LDS (a free column as zeros), the optimal
// assignment (sq_assign_optimal_i32, lane p owning column p), then the clip's twelve figures as wave sums -- lane g < G brings its
// truth's counters, lane p < P its column's --, written by lane 0; a closed lane's figures go into totals and its table is freed,
// every lane storing over the words it read itself.
__global__ __launch_bounds__(64) void k_lane_idf_solve(const LaneIdfSolveArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ int s_w[SQ_SCORE_MAXG * SQ_IDF_MAXP];
  __shared__ int s_r2c[SQ_SCORE_MAXG];
  const SqairLaneIdf& f = a.idf;
  const int b = blockIdx.x, L = threadIdx.x, G = a.G, P = f.P;
  const int cid = L < P ? f.col_id[(size_t)b * P + L] : -1;
  for (int i = L; i < G * P; i += 64) s_w[i] = f.col_id[(size_t)b * P + i % P] >= 0 ? f.overlap[(size_t)b * G * P + i] : 0;
  __syncthreads();
  const long long idtp = sq_assign_optimal_i32(s_w, P, G, P, s_r2c);
  __syncthreads();
  const size_t e = (size_t)b * G + L;
  const int rf = L < G ? f.row_frames[e] : 0, m = L < G ? f.matched[e] : 0;
  const bool traj = rf > 0, mt = traj && 5ll * m >= 4ll * rf, ml = traj && 5ll * m < rf;
  const long long n_row = sq_wave_sum_i64(rf), n_col = sq_wave_sum_i64(cid >= 0 ? f.col_frames[(size_t)b * P + L] : 0);
  const long long n_traj = sq_wave_sum_i64(traj), n_mt = sq_wave_sum_i64(mt), n_ml = sq_wave_sum_i64(ml);
  const long long n_frag = sq_wave_sum_i64(L < G ? f.frag[e] : 0), n_ids = sq_wave_sum_i64(cid >= 0);
  const bool closed = a.close && a.close[b] != 0;
  if (L < G && a.assign) {
    const int p = s_r2c[L];
    a.assign[e] = p >= 0 && s_w[L * P + p] > 0 ? f.col_id[(size_t)b * P + p] : -1;
  }
  if (L == 0) {
    const long long frames = f.frames[b], extra = f.extra_frames[b];
    const long long fig[SQAIR_IDF_TOTALS] = {frames > 0, frames, n_traj, idtp, n_row - idtp, n_col + extra - idtp, n_mt,
                                             n_traj - n_mt - n_ml, n_ml, n_frag, n_ids, 0};
#pragma unroll
    for (int k = 0; k < SQAIR_IDF_TOTALS; ++k) {
      if (a.open) a.open[(size_t)b * SQAIR_IDF_TOTALS + k] = fig[k];
      if (closed) f.totals[(size_t)b * SQAIR_IDF_TOTALS + k] += fig[k];
    }
    if (closed) { f.frames[b] = 0; f.extra_frames[b] = 0; }
  }
  if (!closed) return;
  __syncthreads();   // (assign has read the ids of the columns before they are freed)
  if (L < P) f.col_id[(size_t)b * P + L] = -1;
  if (L < G) { f.row_frames[e] = 0; f.matched[e] = 0; f.frag[e] = 0; f.trk_state[e] = 0; }
}
int sq_launch_lane_idf_solve(const LaneIdfSolveArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_idf_solve, dim3(a.B), dim3(64), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// HOTA scoring (sqair_set_hota; LaneHotaArgs / LaneHotaSolveArgs in sqair_glue.h; the semantics: include/sqair_hip.h, points 1-6)
// ------------------------------------------------------------------------------------------------
// k_lane_hota: workgroup = lane b, looping over the pass's frames in order with the lane's column table in LDS across them.  Per
// scored frame thread 0 takes the next record -- or counts the frame as dropped when the log is full --, finds or makes the column
// of every present lane object (sq_lane_id_column: the IDF's walk) and writes the record's row word; then thread j < N stores its
// object's column and thread i < G * N computes the IoU of pair (g, j) = (i / N, i % N) on the words the score read and stores its
// q: every word of the record is written.  Every branch around a barrier depends on truth_valid[t, b], map_count[t, b] and whether
// the log is full alone: uniform over the workgroup.
__global__ __launch_bounds__(256) void k_lane_hota(const LaneHotaArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ int s_cid[SQ_HOTA_MAXP];
  __shared__ int s_jcol[SQ_MAXN];
  __shared__ int s_rec;
  const SqairLaneScore& o = a.sc;
  const SqairLaneHota& f = a.hota;
  const int b = blockIdx.x, tid = threadIdx.x, G = o.G, N = a.N, P = f.P, L = f.L;
  if (tid < P) s_cid[tid] = f.col_id[(size_t)b * P + tid];
  int frames = tid == 0 ? f.frames[b] : 0, c_drop = 0, c_over = 0;   // (thread 0's)
  for (int t = 0; t < a.T; ++t) {
    const size_t tb = (size_t)t * a.B + b;
    if (o.truth_valid[tb] == 0 || a.map_count[tb] == -1) continue;   // no truth, or a non-finite lane: nothing is touched
    __syncthreads();   // (the table is loaded; the last frame's readers are done with s_jcol and s_rec)
    // ---- the record, the columns of the frame's objects and the truth's row word, one thread
    if (tid == 0) {
      int rec = -1;
      if (frames >= 0 && frames < L) {
        rec = frames++;
        int unkeyed = 0, row = 0;
        for (int j = 0; j < N; ++j) {
          s_jcol[j] = -1;
          if (a.presence[tb * N + j] == 0.0f) continue;
          bool fresh;
          const int col = sq_lane_id_column(s_cid, P, (int)sq_word(a.ids + tb * N + j), s_jcol, j, fresh);
          s_jcol[j] = col >= 0 ? col : -2;
          unkeyed += col < 0;
        }
        for (int g = 0; g < G; ++g) row |= (o.truth_present[tb * G + g] != 0) << g;
        f.log_row[(size_t)b * L + rec] = row;
        c_over += unkeyed > 0;
      } else {
        ++c_drop;
      }
      s_rec = rec;
    }
    __syncthreads();
    const int rec = s_rec;
    if (rec < 0) continue;   // the log is full
    const size_t r = (size_t)b * L + rec;
    if (tid < N) f.log_col[r * N + tid] = s_jcol[tid];
    if (tid < G * N) {
      const int g = tid / N, j = tid - g * N;
      int q = -1;
      if (s_jcol[j] >= 0 && o.truth_present[tb * G + g] != 0) {
        const float* p = o.truth_box + (tb * G + g) * 4;
        const float* w = a.box + (tb * N + j) * 4;
        q = __float2int_rn(sq_box_iou(SqBox{p[0], p[1], p[2], p[3]}, SqBox{w[0], w[1], w[2], w[3]}) * 1048576.0f);
      }
      f.log_q[r * G * N + tid] = q;
    }
  }
  __syncthreads();
  if (tid < P) f.col_id[(size_t)b * P + tid] = s_cid[tid];
  if (tid == 0) {
    f.frames[b] = frames; f.dropped_frames[b] += c_drop;
    f.totals_c[(size_t)b * 4 + 3] += c_over;
  }
}
int sq_launch_lane_hota(const LaneHotaArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_hota, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// k_lane_hota_solve: workgroup = lane b, four wavefronts.
//   pass 1   the records in order, one barrier each (the record at work and the next one in two LDS buffers): thread i < G * N forms
//            R_g and C_j of its pair (g, j) from the record in LDS and adds n to cell (g, col(j)) of pot -- the columns of a record
//            are distinct, so a cell has one writer per record, and the barrier orders the records --; thread g counts its row,
//            thread j its column.  Then gas, one thread per cell.
//   pass 2   the records are independent: wavefront v takes records v, v + 4, ..  It builds the int32 table in its own LDS, calls
//            sq_assign_optimal_i32 on it, and lane g files its matched pair under k = the number of thresholds its q reaches
//            (q >= A_i exactly for i <= (20 q) >> 20): one integer atomic each on the pair histogram work[g][p][k] in global memory
//            and on the lane's tp and loc bins in LDS.  Integer sums: they do not depend on the schedule.
//   figures  one thread per cell turns its bins into mc_i (a suffix sum); then lane i - 1 of wavefront 0 owns threshold i: tp, loc,
//            fn, fp and the three double sums over the cells in index order -- one thread, a fixed order.
// The histogram is read back with device-scope atomic loads: the atomics that filled it were performed in L2.  A column index read
// from the log is used only inside 0..P-1, a record count only inside 0..L: a log the caller wrote cannot index outside LDS.
__device__ __forceinline__ int sq_hota_word(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__global__ __launch_bounds__(256) void k_lane_hota_solve(const LaneHotaSolveArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  constexpr int MAXC = SQ_SCORE_MAXG * SQ_HOTA_MAXP, MAXPAIR = SQ_SCORE_MAXG * 16, BINS = SQ_HOTA_BINS;
  __shared__ long long s_pot[MAXC];
  __shared__ int s_gas[MAXC];
  __shared__ int s_q[2][MAXPAIR], s_col[2][16];
  __shared__ int s_w[4][MAXPAIR], s_r2c[4][SQ_SCORE_MAXG];
  __shared__ int s_rfr[SQ_SCORE_MAXG], s_cfr[SQ_HOTA_MAXP], s_extra, s_tp[BINS];
  __shared__ unsigned long long s_loc[BINS];
  const SqairLaneHota& f = a.hota;
  const int b = blockIdx.x, tid = threadIdx.x, G = a.G, N = a.N, P = f.P, L = f.L, GN = G * N, GP = G * P;
  const int F = min(max(f.frames[b], 0), L);
  int* work = f.work + (size_t)b * GP * BINS;
  for (int i = tid; i < GP; i += 256) s_pot[i] = 0;
  for (int i = tid; i < GP * BINS; i += 256) work[i] = 0;
  if (tid < G) s_rfr[tid] = 0;
  if (tid < P) s_cfr[tid] = 0;
  if (tid < BINS) { s_tp[tid] = 0; s_loc[tid] = 0ull; }
  if (tid == 0) s_extra = 0;
  __threadfence();   // (the zeroes are in L2 before any wavefront's atomics)
  __syncthreads();
  // ---- pass 1
  const int g = tid / N, j = tid - g * N;
  for (int rec = 0; rec < F; ++rec) {
    const size_t r = (size_t)b * L + rec;
    const int buf = rec & 1, row = f.log_row[r];
    if (tid < GN) s_q[buf][tid] = f.log_q[r * GN + tid];
    if (tid < N) s_col[buf][tid] = f.log_col[r * N + tid];
    __syncthreads();   // (record rec is in its buffer; the last record's adds are done)
    if (tid < GN) {
      const int q = s_q[buf][tid], col = s_col[buf][j];
      if (q >= 0 && col >= 0 && col < P) {
        long long R = 0, C = 0;
        for (int jj = 0; jj < N; ++jj) R += max(s_q[buf][g * N + jj], 0);
        for (int gg = 0; gg < G; ++gg) C += max(s_q[buf][gg * N + j], 0);
        const long long den = R + C - q;
        if (den > 0) s_pot[g * P + col] += ((long long)q << 20) / den;
      }
    }
    if (tid < G && ((row >> tid) & 1)) s_rfr[tid] += 1;
    if (tid < N) {
      const int col = s_col[buf][tid];
      if (col >= 0 && col < P) s_cfr[col] += 1;
      else if (col == -2) atomicAdd(&s_extra, 1);
    }
  }
  __syncthreads();
  for (int i = tid; i < GP; i += 256) {
    const long long pot = s_pot[i], den = ((long long)(s_rfr[i / P] + s_cfr[i % P]) << 20) - pot;
    s_gas[i] = den > 0 ? (int)((pot << 20) / den) : 0;
  }
  __syncthreads();
  // ---- pass 2
  const int wv = tid >> 6, ln = tid & 63;
  for (int rec = wv; rec < F; rec += 4) {
    const size_t r = (size_t)b * L + rec;
    for (int i = ln; i < GN; i += 64) {
      const int q = f.log_q[r * GN + i], col = f.log_col[r * N + i % N];
      s_w[wv][i] = (q >= 0 && col >= 0 && col < P) ? (int)(((long long)s_gas[(i / N) * P + col] * q) >> 15) : -1;
    }
    sq_wave_lds_order();
    sq_assign_optimal_i32(s_w[wv], N, G, N, s_r2c[wv]);
    sq_wave_lds_order();
    if (ln < G) {
      const int jm = s_r2c[wv][ln];
      if (a.match) a.match[r * G + ln] = jm;
      if (jm >= 0) {
        const int q = f.log_q[r * GN + ln * N + jm], col = f.log_col[r * N + jm];
        const int k = min((int)((20ll * q) >> 20), BINS - 1);
        atomicAdd(&s_tp[k], 1);
        atomicAdd(&s_loc[k], (unsigned long long)q);
        atomicAdd(&work[(ln * P + col) * BINS + k], 1);
      }
    }
    sq_wave_lds_order();   // (the table and row_to_col are read before the next record overwrites them)
  }
  __threadfence();
  __syncthreads();
  // ---- figures: mc_i = the pairs of the cell with k >= i, in place
  for (int c = tid; c < GP; c += 256) {
    int acc = 0;
    for (int k = BINS - 1; k >= 1; --k) {
      acc += sq_hota_word(work + c * BINS + k);
      __hip_atomic_store(work + c * BINS + k, acc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __threadfence();
  __syncthreads();
  const bool closed = a.close && a.close[b] != 0;
  if (tid < SQAIR_HOTA_ALPHAS) {
    const int i = tid + 1;
    long long tp = 0, loc = 0, n_row = 0, n_col = 0;
    for (int k = i; k < BINS; ++k) { tp += s_tp[k]; loc += (long long)s_loc[k]; }
    for (int gg = 0; gg < G; ++gg) n_row += s_rfr[gg];
    for (int p = 0; p < P; ++p) n_col += s_cfr[p];
    double ass = 0.0, re = 0.0, pr = 0.0;
    for (int c = 0; c < GP; ++c) {
      const int mc = sq_hota_word(work + c * BINS + i);
      if (mc <= 0) continue;
      const int rf = s_rfr[c / P], cf = s_cfr[c % P];
      const double m2 = (double)mc * (double)mc;
      ass += m2 / (double)(rf + cf - mc);
      re += m2 / (double)rf;
      pr += m2 / (double)cf;
    }
    const long long fi[4] = {tp, n_row - tp, n_col + s_extra - tp, loc};
    const double ff[3] = {ass, re, pr};
    const size_t e = (size_t)b * SQAIR_HOTA_ALPHAS + tid;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (a.open_i) a.open_i[e * 4 + k] = fi[k];
      if (closed) f.totals_i[e * 4 + k] += fi[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      if (a.open_f) a.open_f[e * 3 + k] = ff[k];
      if (closed) f.totals_f[e * 3 + k] += ff[k];
    }
  }
  if (tid == 0) {
    const long long fc[4] = {F > 0, F, f.dropped_frames[b], 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (a.open_c) a.open_c[(size_t)b * 4 + k] = fc[k];
      if (closed) f.totals_c[(size_t)b * 4 + k] += fc[k];
    }
    if (closed) { f.frames[b] = 0; f.dropped_frames[b] = 0; }
  }
  if (closed && tid < P) f.col_id[(size_t)b * P + tid] = -1;
}
int sq_launch_lane_hota_solve(const LaneHotaSolveArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_hota_solve, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// The track log (sqair_set_tracklog; LaneTrackLogArgs / LaneTrackLogSmoothArgs in sqair_glue.h; the semantics: include/sqair_hip.h,
// the track log paragraph, points A and 1-5)
// ------------------------------------------------------------------------------------------------
// k_lane_tracklog: workgroup = lane b.  Frame t of the pass takes record (count[b] + t) mod L; the words are copied as they are,
// thread i of the frame's N * 4 box words, N ids, N lengths and one valid word, the frames in order.  Every thread reads count[b]
// before the barrier, thread 0 advances it behind it.  A record index is formed inside 0..L-1 whatever count holds.
__global__ __launch_bounds__(256) void k_lane_tracklog(const LaneTrackLogArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  const SqairLaneTrackLog& f = a.log;
  const int b = blockIdx.x, tid = threadIdx.x, N = a.N, L = f.L;
  const long long c0 = f.count[b];
  int rec = (int)(((c0 % L) + L) % L);
  __syncthreads();
  for (int t = 0; t < a.T; ++t) {
    const size_t tb = (size_t)t * a.B + b, r = (size_t)b * L + rec;
    if (tid < N * 4) sq_put(f.log_box + r * N * 4 + tid, sq_word(a.box + tb * N * 4 + tid));
    if (tid < N) {
      f.log_id[r * N + tid] = a.lane_id[tb * N + tid];
      f.log_len[r * N + tid] = a.track_len[tb * N + tid];
    }
    if (tid == 0) f.log_valid[r] = a.best_row[tb] != -1;
    rec = rec + 1 == L ? 0 : rec + 1;
  }
  if (tid == 0) f.count[b] = c0 + a.T;
}
int sq_launch_lane_tracklog(const LaneTrackLogArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_tracklog, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// k_lane_tracklog_smooth: workgroup = lane b.
//   window   frame f of the window is record (r0 + f) mod L for f >= fmin (fmin = lag - count where the log is younger than the
//            window), "no record" before; it COUNTS when its valid word is set.
//   columns  up to C rounds of a workgroup maximum, "the largest id below the previous one", over the lag * N id words of the
//            frames that count (an integer atomicMax in LDS: no order to depend on); n_tracks counts the id words that no earlier
//            word of the window holds -- each thread walks back from its word and stops at the first sighting it meets.
//   slots    thread i of lag * C finds the slot of column c in frame f (the smallest j) into `work`, and the first and last such
//            frame of the column by integer atomicMin / atomicMax in LDS.
//   filter   thread (column, axis) < 2 C walks the frames forward -- sq_kf_predict, sq_kf_update (sqair_lane.h) on its own five
//            words -- and stores the filtered state; then backward over the stepped frames, reading its own stores back:
//            sq_tracklog_walk (sqair_lane.h), the one statement of it, k_lane_tracklog_stitch's too.
// `work` and filt are global: at the limits neither fits LDS.  What a thread reads of them it wrote itself, but for `work`, which
// is read behind a fence and a barrier.  A slot read from `work` is the one this launch wrote, inside 0..N-1; a record index is
// formed inside 0..L-1.  No arrays in registers but a thread's five words, indexed by constants.
__global__ __launch_bounds__(256) void k_lane_tracklog_smooth(const LaneTrackLogSmoothArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ int s_max[2], s_n, s_desc[SQ_TRACKLOG_MAXC], s_f0[SQ_TRACKLOG_MAXC], s_f1[SQ_TRACKLOG_MAXC];
  const SqairLaneTrackLog& g = a.log;
  const SqairTrackLogOut& o = a.out;
  const int b = blockIdx.x, tid = threadIdx.x, N = a.N, L = g.L, lag = a.lag, C = a.C, B = a.B;
  const long long cnt = max(g.count[b], 0ll), base = cnt - lag;
  const int fmin = base < 0 ? (int)(-base) : 0;                    // the first frame of the window that has a record
  const int r0 = (int)(((base % L) + L) % L);
  const int* lvalid = g.log_valid + (size_t)b * L;
  const int* lid = g.log_id + (size_t)b * L * N;
  auto record = [&](int f) { const int r = r0 + f; return r >= L ? r - L : r; };   // (f < lag <= L)
  auto counts = [&](int f) { return f >= fmin && lvalid[record(f)] != 0; };
  // ---- 1: the window
  for (int f = tid; f < lag; f += 256) o.frame_index[(size_t)f * B + b] = f >= fmin ? base + f : -1ll;
  if (tid < C) { s_desc[tid] = -1; s_f0[tid] = lag; s_f1[tid] = -1; }
  if (tid == 0) s_n = 0;
  // ---- 2: the columns, the largest id first
  int K = 0;
  long long below = 1ll << 31;
  for (int c = 0; c < C; ++c) {
    if (tid == 0) s_max[c & 1] = -1;   // (two words in turn: a thread may still be reading the last round's)
    __syncthreads();
    int best = -1;
    for (int i = tid; i < lag * N; i += 256) {
      const int f = i / N, j = i - f * N;
      if (!counts(f)) continue;
      const int id = lid[(size_t)record(f) * N + j];
      if (id >= 0 && id < below && id > best) best = id;
    }
    if (best >= 0) atomicMax(&s_max[c & 1], best);
    __syncthreads();
    const int m = s_max[c & 1];
    if (m < 0) break;   // (uniform: every thread reads the same word behind the barrier)
    if (tid == 0) s_desc[c] = m;
    below = m;
    K = c + 1;
  }
  // n_tracks: the id words of the window that are a first sighting
  {
    int first = 0;
    for (int i = tid; i < lag * N; i += 256) {
      const int f = i / N, j = i - f * N;
      if (!counts(f)) continue;
      const int id = lid[(size_t)record(f) * N + j];
      if (id < 0) continue;
      bool seen = false;
      for (int jj = 0; jj < j && !seen; ++jj) seen = lid[(size_t)record(f) * N + jj] == id;
      for (int ff = f - 1; ff >= fmin && !seen; --ff) {
        if (lvalid[record(ff)] == 0) continue;
        for (int jj = 0; jj < N && !seen; ++jj) seen = lid[(size_t)record(ff) * N + jj] == id;
      }
      first += !seen;
    }
    if (first) atomicAdd(&s_n, first);
  }
  __syncthreads();   // (s_desc, K columns of it; s_n)
  if (tid == 0) o.n_tracks[b] = s_n;
  if (tid < C) o.track_id[(size_t)b * C + tid] = tid < K ? s_desc[K - 1 - tid] : -1;
  // ---- the slot of every (frame, column), and each column's span
  int* work = a.work + (size_t)b * lag * C;
  for (int i = tid; i < lag * C; i += 256) {
    const int f = i / C, c = i - f * C;
    int slot = -1;
    if (c < K && counts(f)) {
      const int id = s_desc[K - 1 - c];
      const int* w = lid + (size_t)record(f) * N;
      for (int j = N - 1; j >= 0; --j)
        if (w[j] == id) slot = j;
    }
    work[i] = slot;
    if (slot >= 0) { atomicMin(&s_f0[c], f); atomicMax(&s_f1[c], f); }
  }
  __threadfence();
  __syncthreads();
  if (tid < C) {
    int len = -1;
    const int f = tid < K ? s_f0[tid] : lag;
    const int j = f < lag ? work[f * C + tid] : -1;   // (a kept id was seen in the window: f < lag and j >= 0, checked all the same)
    if (j >= 0) len = g.log_len[((size_t)b * L + record(f)) * N + j];
    o.len0[(size_t)b * C + tid] = len;
  }
  if (tid >= C * 2) return;   // (no barrier below)
  // ---- 3, 4: forward and backward, thread = (column, axis): the walk of sqair_lane.h, on this launch's own slots
  const int c = tid >> 1, ax = tid & 1;
  const int f0 = c < K ? s_f0[c] : lag, f1 = c < K ? s_f1[c] : -1;
  sq_tracklog_walk(o, work, g.log_box + (size_t)b * L * N * 4, counts, record, f0, f1, b, c, ax, lag, B, C, N, a.q, a.r, a.v0_var);
}
int sq_launch_lane_tracklog_smooth(const LaneTrackLogSmoothArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_tracklog_smooth, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Track log scoring (sqair_lane_tracklog_score; LaneTrackLogScoreArgs in sqair_glue.h; the semantics: include/sqair_hip.h, the track
// log scoring paragraph, points 1-7)
// ------------------------------------------------------------------------------------------------
// k_lane_tracklog_score: workgroup = lane b, wavefront v = view v of the solve's table (src = v & 1, fill = v >> 1).  The identity
// memory makes the frames serial, the four views share nothing: each wavefront walks the window on its own, with its own tables in
// LDS (SqTrackLogScoreWave, 13.25 KiB a wave) and no workgroup barrier anywhere.  Per scored frame the wave's lanes stage the columns'
// and the truths' presence, lane i fills entries i, i + 64, .. of the G x C IoU table (-1 for a pair that is no candidate) and counts
// the entry into the overlap table when it passes; lane 0 walks sq_assign_keep_greedy, or the whole wave sq_assign_keep_optimal -- the
// branch is on a kernel argument --; lane 0 counts the events, keeping the view's counters and sums as scalars; lanes g < G write the
// per-frame outputs.  After the window the wave solves the overlap table (sq_assign_optimal_i32).  Whether a frame is scored is read
// by every lane from the same words and made a scalar (readfirstlane), so the wave-wide functions are called by all 64 lanes.
// Between a lane's LDS stores and another lane's loads stands sq_wave_lds_order (sqair_lane.h): a wavefront's LDS instructions
// execute in program order.  Nothing is indexed in registers; every index is formed inside the table: f < lag, c < C, g < G, the
// record inside 0..L-1.
struct SqTrackLogScoreWave {
  float iou[SQ_SCORE_MAXG * SQ_TRACKLOG_MAXC];
  int w[SQ_SCORE_MAXG * SQ_TRACKLOG_MAXC];     // sq_assign_keep_optimal's own table
  int ov[SQ_SCORE_MAXG * SQ_TRACKLOG_MAXC];
  int cid[SQ_TRACKLOG_MAXC], cpres[SQ_TRACKLOG_MAXC], cgap[SQ_TRACKLOG_MAXC], claim[SQ_TRACKLOG_MAXC];
  int last[SQ_SCORE_MAXG], tpres[SQ_SCORE_MAXG], rm[SQ_SCORE_MAXG], assign[SQ_SCORE_MAXG];
};
__global__ __launch_bounds__(256) void k_lane_tracklog_score(const LaneTrackLogScoreArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ SqTrackLogScoreWave s_view[SQAIR_TRACKLOG_SCORE_VIEWS];
  const int b = blockIdx.x, v = threadIdx.x >> 6, L = threadIdx.x & 63;
  SqTrackLogScoreWave& s = s_view[v];
  const SqairTrackLogOut& t = a.tab;
  const SqairTrackLogTruth& tr = a.tr;
  const SqairTrackLogScore& o = a.sc;
  const int lag = a.lag, C = a.C, B = a.B, G = tr.G, LR = a.log.L;
  const bool fill = (v >> 1) != 0;
  const float* src = (v & 1) ? t.smooth : t.filt;
  const float iou_min = o.iou_min;
  const int* lvalid = a.log.log_valid + (size_t)b * LR;
  if (L < C) s.cid[L] = t.track_id[(size_t)b * C + L];
  if (L < G) s.last[L] = -1;
  for (int i = L; i < G * C; i += 64) s.ov[i] = 0;
  long long c_frames = 0, c_invalid = 0, c_truth = 0, c_tp = 0, c_fn = 0, c_fp = 0, c_idsw = 0, c_gtp = 0, c_gfp = 0, c_nn = 0, c_gnn = 0;
  double iou_sum = 0.0, err_sum = 0.0, nees_sum = 0.0, gerr_sum = 0.0, gnees_sum = 0.0;
  for (int f = 0; f < lag; ++f) {
    const size_t fb = (size_t)f * B + b;
    const long long fi = t.frame_index[fb];
    const bool truth = tr.truth_valid[fb] != 0;
    const bool finite = fi >= 0 && lvalid[(int)(fi % LR)] != 0;
    const int kind = __builtin_amdgcn_readfirstlane(fi < 0 || !truth ? 0 : finite ? 2 : 1);   // 0 nothing, 1 frames_invalid, 2 scored
    sq_wave_lds_order();   // (the last frame's readers are done with the tables)
    if (kind != 2) {
      c_invalid += kind;
      if (L < G) {
        const size_t e = (((size_t)v * lag + f) * B + b) * G + L;
        if (o.match) o.match[e] = -1;
        if (o.match_iou) o.match_iou[e] = 0.0f;
      }
      continue;
    }
    // ---- 1, 3: presence on both sides, the candidates' IoU, the overlap table
    if (L < C) {
      const int st = t.state[fb * C + L];
      s.cpres[L] = st == 1 || (fill && st == 2);
      s.cgap[L] = st == 2;
    }
    if (L < G) s.tpres[L] = tr.truth_present[fb * G + L] != 0;
    sq_wave_lds_order();
    for (int i = L; i < G * C; i += 64) {
      const int g = i / C, c = i - g * C;
      float q = -1.0f;
      if (s.tpres[g] && s.cpres[c]) {
        const float* p = tr.truth_box + (fb * G + g) * 4;
        const size_t e = (fb * C + c) * 2;
        const float h = t.size[e], w = t.size[e + 1];
        q = sq_box_iou(SqBox{p[0], p[1], p[2], p[3]}, SqBox{fmaf(-0.5f, h, src[e * 5]), fmaf(-0.5f, w, src[(e + 1) * 5]), h, w});
      }
      s.iou[i] = q;
      if (q >= iou_min) s.ov[i] += 1;
    }
    sq_wave_lds_order();
    // ---- 3: the assignment
    if (a.match) sq_assign_keep_optimal(s.iou, C, G, C, iou_min, s.last, s.cid, s.rm, s.claim, s.w);
    else if (L == 0) sq_assign_keep_greedy(s.iou, C, G, C, iou_min, s.last, s.cid, s.rm, s.claim);
    sq_wave_lds_order();
    // ---- 3, 4: the events and the pairs' errors, one lane
    if (L == 0) {
      int n_truth = 0, tp = 0, fn = 0, fp = 0, sw = 0, gtp = 0, gfp = 0, nn = 0, gnn = 0;
      for (int g = 0; g < G; ++g) {
        if (!s.tpres[g]) continue;
        ++n_truth;
        const int c = s.rm[g];
        if (c < 0) { ++fn; continue; }
        ++tp;
        const int id = s.cid[c], last = s.last[g];
        sw += last >= 0 && last != id;
        s.last[g] = id;
        iou_sum += (double)s.iou[g * C + c];
        const float* p = tr.truth_box + (fb * G + g) * 4;
        const float* ky = src + (fb * C + c) * 10;
        const float ty = fmaf(0.5f, p[2], p[0]), tx = fmaf(0.5f, p[3], p[1]);
        const float dy = ty - ky[0], dx = tx - ky[5];
        const float err = sqrtf(fmaf(dy, dy, dx * dx));
        const float ppy = ky[2], ppx = ky[7];
        const bool honest = ppy > 0.0f && ppx > 0.0f;   // (a NaN fails)
        const float nees = dy * dy / ppy + dx * dx / ppx;
        const bool gap = s.cgap[c] != 0;
        err_sum += (double)err;
        if (honest) { nees_sum += (double)nees; ++nn; }
        if (gap) {
          ++gtp;
          gerr_sum += (double)err;
          if (honest) { gnees_sum += (double)nees; ++gnn; }
        }
      }
      for (int c = 0; c < C; ++c) {
        const bool un = s.cpres[c] && !s.claim[c];
        fp += un;
        gfp += un && s.cgap[c];
      }
      ++c_frames; c_truth += n_truth; c_tp += tp; c_fn += fn; c_fp += fp; c_idsw += sw; c_gtp += gtp; c_gfp += gfp; c_nn += nn; c_gnn += gnn;
    }
    if (L < G) {
      const size_t e = (((size_t)v * lag + f) * B + b) * G + L;
      const int c = s.rm[L];
      if (o.match) o.match[e] = c;
      if (o.match_iou) o.match_iou[e] = c >= 0 ? s.iou[L * C + c] : 0.0f;
    }
  }
  // ---- 5: the window's identity assignment
  sq_wave_lds_order();
  const long long idtp = sq_assign_optimal_i32(s.ov, C, G, C, s.assign);
  sq_wave_lds_order();
  if (L < G && o.assign) {
    const int c = s.assign[L];
    o.assign[((size_t)v * B + b) * G + L] = c >= 0 && s.ov[L * C + c] > 0 ? c : -1;
  }
  if (L == 0) {
    int64_t* c = o.counts + ((size_t)b * SQAIR_TRACKLOG_SCORE_VIEWS + v) * SQAIR_TRACKLOG_SCORE_COUNTS;
    c[0] = c_frames; c[1] = c_invalid; c[2] = c_truth; c[3] = c_tp; c[4] = c_fn; c[5] = c_fp; c[6] = c_idsw; c[7] = c_gtp; c[8] = c_gfp;
    c[9] = c_nn; c[10] = c_gnn; c[11] = idtp; c[12] = c_truth - idtp; c[13] = c_tp + c_fp - idtp;   // (tp + fp: the present columns)
    double* d = o.sums + ((size_t)b * SQAIR_TRACKLOG_SCORE_VIEWS + v) * SQAIR_TRACKLOG_SCORE_SUMS;
    d[0] = iou_sum; d[1] = err_sum; d[2] = nees_sum; d[3] = gerr_sum; d[4] = gnees_sum;
  }
}
int sq_launch_lane_tracklog_score(const LaneTrackLogScoreArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_tracklog_score, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Motion calibration (sqair_lane_tracklog_fit; LaneTrackLogFitArgs in sqair_glue.h; the semantics: include/sqair_hip.h, the track log
// fit paragraph, points 1-5)
// ------------------------------------------------------------------------------------------------
// k_lane_tracklog_fit: workgroup = (lane b, iq); its R candidates go in rounds of per = 256 / (2 C) at a time, thread = (candidate of
// the round, column, axis): per * 2 C <= 256 threads walk, the rest idle (2 C need not divide 256).  The serial chain is lag steps a
// thread; what a step reads -- the state word of (frame, column) and z of (frame, column, axis) -- does not depend on the candidate,
// so the workgroup stages it in LDS for SQ_FIT_FRAMES frames at a time, all 256 threads, one (frame, column) each: the state, the
// slot from `work`, the record from frame_index, the box words, z for both axes.  The walk then reads LDS only: threads of one
// candidate read consecutive words, threads of different candidates the same word.  One code path for every lag and C.  A thread
// keeps its five state words, three counters and four fp64 sums in registers, adding in frame order; after the window they go to
// LDS, and thread i < per adds candidate i's 2 C partial sums in (c, a) index order and writes the candidate's words.  Every barrier
// stands under conditions on kernel arguments alone.  LDS: 16 KiB z, 8 KiB states, 8 KiB + 3 KiB partial sums.
// Indices: state and work inside [lag][C] of lane b; a slot is used only inside 0..N-1 and with a frame_index >= 0, the record is
// formed inside 0..L-1 (a state 1 without either is no table of the solve's and is walked as state 0); iq < Q and ir < R <= 16.
constexpr int SQ_FIT_FRAMES = 32;
__global__ __launch_bounds__(256) void k_lane_tracklog_fit(const LaneTrackLogFitArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ float s_z[SQ_FIT_FRAMES * 2 * SQ_TRACKLOG_MAXC];
  __shared__ int s_st[SQ_FIT_FRAMES * SQ_TRACKLOG_MAXC];
  __shared__ double s_sum[256 * SQAIR_TRACKLOG_FIT_SUMS];
  __shared__ int s_cnt[256 * SQAIR_TRACKLOG_FIT_COUNTS];
  const SqairTrackLogOut& t = a.tab;
  const SqairTrackLogFit& o = a.fit;
  const int b = blockIdx.x, iq = blockIdx.y, tid = threadIdx.x;
  const int lag = a.lag, C = a.C, N = a.N, B = a.B, LR = a.log.L, R = o.R, C2 = 2 * C, burn = o.burn;
  const int per = 256 / C2;
  const float q = o.q[iq], v0_var = o.v0_var;
  const int32_t* work = a.work + (size_t)b * lag * C;
  const float* lbox = a.log.log_box + (size_t)b * LR * N * 4;
  const int lr = tid / C2, ca = tid - lr * C2, c = ca >> 1;
  for (int r0 = 0; r0 < R; r0 += per) {
    const int ir = r0 + lr;
    const bool mine = lr < per && ir < R;
    const float r = o.r[mine ? ir : 0];
    float2* innov = mine && iq == 0 && ir == 0 && o.innov ? (float2*)o.innov : nullptr;   // candidate (0, 0) writes every word of it
    float k[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    bool started = false, gap = false;
    int i = 0, n = 0, n_gap = 0, skipped = 0;
    double nis_sum = 0.0, lns_sum = 0.0, gnis_sum = 0.0, glns_sum = 0.0;
    for (int f0 = 0; f0 < lag; f0 += SQ_FIT_FRAMES) {
      const int nf = min(SQ_FIT_FRAMES, lag - f0);
      __syncthreads();   // (the last block's walkers are done with the staged words)
      for (int e = tid; e < nf * C; e += 256) {
        const int fl = e / C, cc = e - fl * C, f = f0 + fl;
        const size_t fb = (size_t)f * B + b;
        int st = t.state[fb * C + cc];
        float zy = 0.0f, zx = 0.0f;
        if (st == 1) {
          const long long fi = t.frame_index[fb];
          const int j = work[f * C + cc];
          if (fi >= 0 && j >= 0 && j < N) {
            const float* p = lbox + ((size_t)(fi % LR) * N + j) * 4;
            zy = fmaf(0.5f, p[2], p[0]);
            zx = fmaf(0.5f, p[3], p[1]);
          } else {
            st = 0;
          }
        }
        s_st[e] = st;
        s_z[e * 2] = zy;
        s_z[e * 2 + 1] = zx;
      }
      __syncthreads();
      if (!mine) continue;   // (the barriers are the loop's, above)
      for (int fl = 0; fl < nf; ++fl) {
        const int st = s_st[fl * C + c];
        const float z = s_z[fl * C2 + ca];
        float y = 0.0f, S = 0.0f;
        if (st == 1 && !started) {
          k[0] = z; k[1] = 0.0f; k[2] = r; k[3] = 0.0f; k[4] = v0_var;
          started = true; gap = false; i = 0;
        } else if (st == 1) {
          S = sq_kf_predict(k, q, r);
          y = z - k[0];
          const float nis = (y * y) / S;
          ++i;
          if (i > burn) {
            if (S > 0.0f && isfinite(nis)) {
              const double dn = (double)nis, dl = log((double)S);
              ++n; nis_sum += dn; lns_sum += dl;
              if (gap) { ++n_gap; gnis_sum += dn; glns_sum += dl; }
            } else {
              ++skipped;
            }
          }
          sq_kf_update(k, S, z);
          gap = false;
        } else if (st == 2 && started) {
          sq_kf_predict(k, q, r);
          gap = true;
        }
        if (innov) innov[(((size_t)(f0 + fl) * B + b) * C + c) * 2 + (ca & 1)] = make_float2(y, S);
      }
    }
    s_sum[tid * 4] = nis_sum; s_sum[tid * 4 + 1] = lns_sum; s_sum[tid * 4 + 2] = gnis_sum; s_sum[tid * 4 + 3] = glns_sum;
    s_cnt[tid * 3] = n; s_cnt[tid * 3 + 1] = n_gap; s_cnt[tid * 3 + 2] = skipped;
    __syncthreads();
    if (tid < per && r0 + tid < R) {
      long long cn = 0, cg = 0, cs = 0;
      double d0 = 0.0, d1 = 0.0, d2 = 0.0, d3 = 0.0;
      for (int j = tid * C2; j < (tid + 1) * C2; ++j) {
        cn += s_cnt[j * 3]; cg += s_cnt[j * 3 + 1]; cs += s_cnt[j * 3 + 2];
        d0 += s_sum[j * 4]; d1 += s_sum[j * 4 + 1]; d2 += s_sum[j * 4 + 2]; d3 += s_sum[j * 4 + 3];
      }
      const size_t e = ((size_t)b * o.Q + iq) * R + r0 + tid;
      int64_t* cw = o.counts + e * SQAIR_TRACKLOG_FIT_COUNTS;
      cw[0] = cn; cw[1] = cg; cw[2] = cs;
      double* dw = o.sums + e * SQAIR_TRACKLOG_FIT_SUMS;
      dw[0] = d0; dw[1] = d1; dw[2] = d2; dw[3] = d3;
    }
    __syncthreads();   // (the partial sums are read before the next round's walkers can write theirs)
  }
}
int sq_launch_lane_tracklog_fit(const LaneTrackLogFitArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_tracklog_fit, dim3(a.B, a.fit.Q), dim3(256), 0, s, a);
  return 0;
}

// ------------------------------------------------------------------------------------------------
// Track log stitching (sqair_lane_tracklog_stitch; LaneTrackLogStitchArgs in sqair_glue.h; the semantics: include/sqair_hip.h, the
// track log stitching paragraph, points 1-7)
// ------------------------------------------------------------------------------------------------
// k_lane_tracklog_stitch: workgroup = lane b, 256 threads.
//   window   the solve's own: record(f) and counts(f) from count, L and log_valid; s_pre[f] = the counting frames below f (thread t
//            counts frames 16 t .. 16 t + 15, then adds the partial counts below it: lag <= 4096 = 256 * 16), so that a gap is a
//            difference of two words.
//   spans    thread i of lag * C: integer atomicMin / atomicMax in LDS over the frames with state != 0.
//   table    thread i of C * C = (predecessor, successor): the candidate test in integers, then sq_stitch_d2 (sqair_lane.h) on the
//            predecessor's filtered words at f1 and the successor's smoothed words at f0 -- global, read-only, the solve's -- and the
//            weight into s_w.  Wave 0 calls sq_assign_optimal_i32 on it; the branch is wave-uniform.
//   chains   thread c < C: its link (taken only with a positive weight), its root by walking s_prev (at most C steps), the root's
//            rank among the roots = the stitched column; a root walks s_next to the chain's last fragment.
//   slots    thread i of lag * C = (frame, stitched column) walks its chain to the fragment whose span holds the frame and copies
//            that `work` word into work_out (inside 0..N-1, else -1): one writer per word.
//   filter   behind a fence and a barrier, thread (stitched column, axis) < 2 C: sq_tracklog_walk on work_out, as the solve.
// Every barrier stands under conditions on kernel arguments alone.  Indices: f < lag, columns < C -- what the solver returns is
// checked against 0..C-1 before it is used --, s_pre inside 0..lag, a record inside 0..L-1, a slot inside 0..N-1.  No arrays in
// registers but five state words indexed by constants.  LDS: 16 KiB weights, 8 KiB s_pre, 3 KiB the rest.
constexpr int SQ_STITCH_CHUNK = SQ_TRACKLOG_MAXL / 256;
__global__ __launch_bounds__(256) void k_lane_tracklog_stitch(const LaneTrackLogStitchArgs a SQ_TLP) {
  SQ_TL_SCOPE;
  __shared__ int s_w[SQ_TRACKLOG_MAXC * SQ_TRACKLOG_MAXC];
  __shared__ unsigned short s_pre[SQ_TRACKLOG_MAXL + 1];
  __shared__ int s_part[256];
  __shared__ int s_id[SQ_TRACKLOG_MAXC], s_f0[SQ_TRACKLOG_MAXC], s_f1[SQ_TRACKLOG_MAXC], s_next[SQ_TRACKLOG_MAXC], s_prev[SQ_TRACKLOG_MAXC];
  __shared__ int s_rootof[SQ_TRACKLOG_MAXC], s_last[SQ_TRACKLOG_MAXC], s_tot[2];
  const SqairLaneTrackLog& g = a.log;
  const SqairTrackLogOut& t = a.tab;
  const SqairTrackLogOut& o = a.out;
  const SqairTrackLogStitch& st = a.st;
  const int b = blockIdx.x, tid = threadIdx.x, N = a.N, L = g.L, lag = a.lag, C = a.C, B = a.B;
  const long long cnt = max(g.count[b], 0ll), base = cnt - lag;
  const int fmin = base < 0 ? (int)(-base) : 0;                    // the first frame of the window that has a record
  const int r0 = (int)(((base % L) + L) % L);
  const int* lvalid = g.log_valid + (size_t)b * L;
  auto record = [&](int f) { const int r = r0 + f; return r >= L ? r - L : r; };   // (f < lag <= L)
  auto counts = [&](int f) { return f >= fmin && lvalid[record(f)] != 0; };
  const float gate2 = st.gate * st.gate;
  const int32_t* work = a.work + (size_t)b * lag * C;
  // ---- the window: the counting frames below every frame
  const int lo = min(tid * SQ_STITCH_CHUNK, lag), hi = min(lo + SQ_STITCH_CHUNK, lag);
  {
    int n = 0;
    for (int f = lo; f < hi; ++f) n += counts(f);
    s_part[tid] = n;
  }
  if (tid < C) { s_id[tid] = t.track_id[(size_t)b * C + tid]; s_f0[tid] = lag; s_f1[tid] = -1; s_next[tid] = -1; s_prev[tid] = -1; }
  __syncthreads();
  {
    int off = 0;
    for (int i = 0; i < tid; ++i) off += s_part[i];
    for (int f = lo; f < hi; ++f) { s_pre[f] = (unsigned short)off; off += counts(f); }
    if (lo < lag && hi == lag) s_pre[lag] = (unsigned short)off;
  }
  // ---- 1: the fragments' spans; 6: frame_index
  for (int i = tid; i < lag * C; i += 256) {
    const int f = i / C, c = i - f * C;
    if (t.state[((size_t)f * B + b) * C + c] != 0) { atomicMin(&s_f0[c], f); atomicMax(&s_f1[c], f); }
  }
  for (int f = tid; f < lag; f += 256) o.frame_index[(size_t)f * B + b] = t.frame_index[(size_t)f * B + b];
  __syncthreads();
  // ---- 2, 3, 4: the candidates, their distance, the weights
  for (int i = tid; i < C * C; i += 256) {
    const int ca = i / C, cb = i - ca * C;
    const int fa = s_f1[ca], fb = s_f0[cb];
    int w = -1;
    if (ca != cb && s_id[ca] >= 0 && s_id[cb] >= 0 && fa >= 0 && fb < lag && fa < fb && t.len0[(size_t)b * C + cb] == 1) {
      const int gap = (int)s_pre[fb] - (int)s_pre[fa + 1], steps = (int)s_pre[fb + 1] - (int)s_pre[fa + 1];
      if (gap <= st.max_gap) {
        bool ok;
        const float d2 = sq_stitch_d2(t.filt + (((size_t)fa * B + b) * C + ca) * 10, t.smooth + (((size_t)fb * B + b) * C + cb) * 10, steps,
                                      a.q, a.r, gate2, ok);
        if (ok) w = (1 << 28) + min(max(__float2int_rn((1.0f - d2 / gate2) * 1048576.0f), 0), 1 << 20);
      }
    }
    s_w[i] = w;
  }
  __syncthreads();
  if (tid < 64) sq_assign_optimal_i32(s_w, C, C, C, s_next);
  __syncthreads();
  // ---- 5: the links (a pair of weight -1 is never taken; checked all the same), then the chains
  int nx = -1;
  if (tid < C) {
    nx = s_next[tid];
    if (nx < 0 || nx >= C || s_w[tid * C + nx] <= 0) nx = -1;
  }
  __syncthreads();   // (every s_next word is read before any is rewritten)
  if (tid < C) {
    s_next[tid] = nx;
    if (nx >= 0) s_prev[nx] = tid;   // (one to one: one writer)
  }
  __syncthreads();
  if (tid < C) {
    int idx = -1;
    if (s_id[tid] >= 0) {
      int rt = tid;
      for (int i = 0; i < C && s_prev[rt] >= 0; ++i) rt = s_prev[rt];
      idx = 0;
      for (int cc = 0; cc < rt; ++cc) idx += s_id[cc] >= 0 && s_prev[cc] < 0;
      if (rt == tid) {
        int last = tid;
        for (int i = 0; i < C && s_next[last] >= 0; ++i) last = s_next[last];
        s_rootof[idx] = tid;
        s_last[idx] = last;
      }
    }
    // ---- 7: the link outputs
    const size_t e = (size_t)b * C + tid;
    float d2 = 0.0f;
    int gap = -1;
    if (nx >= 0) {
      const int fa = s_f1[tid], fb = s_f0[nx];
      bool ok;
      gap = (int)s_pre[fb] - (int)s_pre[fa + 1];
      d2 = sq_stitch_d2(t.filt + (((size_t)fa * B + b) * C + tid) * 10, t.smooth + (((size_t)fb * B + b) * C + nx) * 10,
                        (int)s_pre[fb + 1] - (int)s_pre[fa + 1], a.q, a.r, gate2, ok);
    }
    st.root[e] = idx;
    st.link_next[e] = nx;
    st.link_d2[e] = d2;
    st.link_gap[e] = gap;
  }
  if (tid == 0) {
    int links = 0, roots = 0;
    for (int c = 0; c < C; ++c) { links += s_next[c] >= 0; roots += s_id[c] >= 0 && s_prev[c] < 0; }
    s_tot[0] = links; s_tot[1] = roots;
  }
  __syncthreads();
  // ---- 6: the stitched table: one column per chain, in the order of the roots
  const int K = s_tot[1];
  if (tid == 0) { st.n_links[b] = s_tot[0]; o.n_tracks[b] = t.n_tracks[b] - s_tot[0]; }
  if (tid < C) {
    const int rc = tid < K ? s_rootof[tid] : -1;
    o.track_id[(size_t)b * C + tid] = rc >= 0 ? s_id[rc] : -1;
    o.len0[(size_t)b * C + tid] = rc >= 0 ? t.len0[(size_t)b * C + rc] : -1;
  }
  int* wout = a.work_out + (size_t)b * lag * C;
  for (int i = tid; i < lag * C; i += 256) {
    const int f = i / C, c = i - f * C;
    int slot = -1;
    if (c < K) {
      int fr = s_rootof[c];
      for (int n = 0; n < C && fr >= 0; ++n) {
        if (f >= s_f0[fr] && f <= s_f1[fr]) {
          const int j = work[f * C + fr];
          slot = j >= 0 && j < N ? j : -1;
          break;
        }
        fr = s_next[fr];
      }
    }
    wout[i] = slot;
  }
  __threadfence();
  __syncthreads();
  if (tid >= C * 2) return;   // (no barrier below)
  const int c = tid >> 1, ax = tid & 1;
  const int f0 = c < K ? s_f0[s_rootof[c]] : lag, f1 = c < K ? s_f1[s_last[c]] : -1;
  sq_tracklog_walk(o, wout, g.log_box + (size_t)b * L * N * 4, counts, record, f0, f1, b, c, ax, lag, B, C, N, a.q, a.r, a.v0_var);
}
int sq_launch_lane_tracklog_stitch(const LaneTrackLogStitchArgs& a, hipStream_t s) {
  SQ_LAUNCH(k_lane_tracklog_stitch, dim3(a.B), dim3(256), 0, s, a);
  return 0;
}
