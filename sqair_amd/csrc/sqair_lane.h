// Device functions of the per-lane answers (sqair_lane.hip): what turns a lane's K particle rows into one answer -- the weights, the
// best row's objects, the association of every particle with them -- stated once for the kernels that need it.
#pragma once
#include "sqair_glue.h"

// The weights of a lane's K particles: a_k accumulated in frame order, m = max a_k, e_k = expf(a_k - m), S = sum e_k and
// Q = sum e_k^2 as ONE thread's loops in index order, ESS = S^2 / Q.  A NaN or +inf a_k, or every a_k at -inf, makes S non-finite.
template <bool MAY_BE_NULL>   // log_w == NULL: zeros (the resampler's is never NULL)
__device__ __forceinline__ float sq_lane_log_weight(const float* log_w, const float* lw, int n_frames, int R, int r) {
  float acc = MAY_BE_NULL && !log_w ? 0.0f : log_w[r];
  for (int t = 0; t < n_frames; ++t) acc += lw[(size_t)t * R + r];
  return acc;
}
__device__ __forceinline__ float sq_lane_max(const float* a, int K) {
  float m = a[0];
  for (int i = 1; i < K; ++i) m = fmaxf(m, a[i]);
  return m;
}
__device__ __forceinline__ float sq_lane_exp(float a, float m) { return expf(a - m); }
template <bool PREFIX>   // PREFIX: e_k is replaced by the inclusive prefix sum c_k (the resampler searches it)
__device__ __forceinline__ void sq_lane_sums(float* e, int K, float& S, float& Q) {
  float c = 0.0f, q = 0.0f;
  for (int i = 0; i < K; ++i) {
    const float v = e[i];
    c += v;
    q += v * v;
    if (PREFIX) e[i] = c;
  }
  S = c;
  Q = q;
}
__device__ __forceinline__ float sq_lane_ess(float S, float Q) { return S * S / Q; }
// sum_k w_k canvas[row0 + k][p], k in index order
__device__ __forceinline__ float sq_lane_mean_pixel(const float* w, const float* __restrict__ canvas, size_t row0, int P, int p, int K) {
  float acc = 0.0f;
  for (int k = 0; k < K; ++k) acc += w[k] * canvas[(row0 + k) * P + p];
  return acc;
}
// The sequence over a workgroup of >= K threads, thread k < K holding a_k (`acc`).  Leaves in s_w[0..K), behind a barrier,
//   PREFIX   the inclusive prefix sums c_k of e_k (nothing is divided; st.best is not formed);
//   else     w_k = e_k / S, and in st.best the first k of maximal a_k (an integer atomicMin in LDS) -- or -1 for a non-finite
//            lane (S not finite): NaN weights, no best row, no objects;
// and in `st` m, S and Q.
struct SqLaneStats { float m, S, Q; int best; };
template <bool PREFIX>
__device__ __forceinline__ void sq_lane_weights(const float acc, const int K, float* s_w, SqLaneStats& st) {
  const int k = threadIdx.x;
  if (k < K) s_w[k] = acc;
  if (k == 0) st.best = K;
  __syncthreads();
  if (k == 0) st.m = sq_lane_max(s_w, K);
  __syncthreads();
  if (k < K) {
    s_w[k] = sq_lane_exp(acc, st.m);
    if (!PREFIX && acc == st.m) atomicMin(&st.best, k);
  }
  __syncthreads();
  if (k == 0) {
    sq_lane_sums<PREFIX>(s_w, K, st.S, st.Q);
    if (!PREFIX && !isfinite(st.S)) st.best = -1;
  }
  __syncthreads();
  if (PREFIX) return;
  if (k < K) s_w[k] = s_w[k] / st.S;
  __syncthreads();
}

// 32-bit words copied as they are
__device__ __forceinline__ unsigned sq_word(const float* p) { return *reinterpret_cast<const unsigned*>(p); }
__device__ __forceinline__ void sq_put(float* p, unsigned v) { *reinterpret_cast<unsigned*>(p) = v; }

// slot 0 of row `row` of a view, in slots
__device__ __forceinline__ size_t sq_lane_slot(const LaneRows& v, size_t row, int N) { return row * v.row_step * N; }

struct SqBox { float y, x, h, w; };
__device__ __forceinline__ float sq_box_coord(const SqBox& b, int c) { return c == 0 ? b.y : c == 1 ? b.x : c == 2 ? b.h : b.w; }
// stn_to_pixel_coords(to_coords(where), (H, W)) (sqair/modules.py:221-262), with the to_coords of the crop and insert kernels
__device__ __forceinline__ SqBox sq_box_of_where(const float* __restrict__ wl, int H, int W) {
  const float sx = sq_to_coord(wl[0], 0), sy = sq_to_coord(wl[1], 1), tx = sq_to_coord(wl[2], 2), ty = sq_to_coord(wl[3], 3);
  SqBox o;
  o.y = 0.5f * (float)(H - 1) * (ty - sy + 1.0f);
  o.x = 0.5f * (float)(W - 1) * (tx - sx + 1.0f);
  o.h = (float)(H + 1) * sy;
  o.w = (float)(W + 1) * sx;
  return o;
}
// axis-aligned intersection over union; 0 when the union is not positive, exactly 1 for the same four words (positive area)
__device__ __forceinline__ float sq_box_iou(const SqBox& p, const SqBox& q) {
  const float oy = fmaxf(fminf(p.y + p.h, q.y + q.h) - fmaxf(p.y, q.y), 0.0f);
  const float ox = fmaxf(fminf(p.x + p.w, q.x + q.w) - fmaxf(p.x, q.x), 0.0f);
  const float inter = oy * ox, uni = p.h * p.w + q.h * q.w - inter;
  if (!(uni > 0.0f)) return 0.0f;
  if (p.y == q.y && p.x == q.x && p.h == q.h && p.w == q.w) return 1.0f;
  return inter / uni;
}

// The best row's objects: thread j < N takes slot j of row `best` of the view (LaneRows, sqair_glue.h) -- absent in a non-finite lane
// (`bad`) -- into s_bp[j] / s_bbox[j] and, where bound, its words and its pixel box into element e0 + j of the outputs.  Ends on a
// barrier.
struct SqBestOut { float* presence; float* obj_id; float* where; float* box; };   // [.., N], [.., N], [.., N, 4], [.., N, 4] or NULL
__device__ __forceinline__ void sq_lane_best_objects(const LaneRows& v, const size_t best, const bool bad, const int N, const int H,
                                                     const int W, const size_t e0, const SqBestOut& o, int* s_bp, SqBox* s_bbox) {
  const int j = threadIdx.x;
  if (j < N) {
    const size_t sl = sq_lane_slot(v, best, N) + j;
    const bool pj = !bad && v.presence[sl * v.pres_ld] != 0.0f;
    SqBox bx = {0.0f, 0.0f, 0.0f, 0.0f};
    if (pj) bx = sq_box_of_where(v.where + sl * v.where_ld, H, W);
    s_bp[j] = pj;
    s_bbox[j] = bx;
    const size_t e = e0 + j;
    if (o.presence) sq_put(o.presence + e, pj ? sq_word(v.presence + sl * v.pres_ld) : 0u);
    if (o.obj_id) sq_put(o.obj_id + e, pj ? sq_word(v.obj_id + sl * v.id_ld) : 0u);
    if (o.where)
      for (int q = 0; q < 4; ++q) sq_put(o.where + e * 4 + q, pj ? sq_word(v.where + sl * v.where_ld + q) : 0u);
    if (o.box) {
      o.box[e * 4 + 0] = bx.y; o.box[e * 4 + 1] = bx.x; o.box[e * 4 + 2] = bx.h; o.box[e * 4 + 3] = bx.w;
    }
  }
  __syncthreads();
}

// The association of ONE particle (the calling thread's row `row` of the view) with the best row's objects: per object j the first
// present slot of maximal IoU, kept in registers -- statically indexed: the j loops are unrolled over the build's slot limit -- and
// left in match[0..N) as a byte (the slot, or 255: below iou_min or no best-row object j).  WITH_ID: fm[j] says whether j is
// matched and fid[j] is the obj_id word of the matched slot (0 otherwise).  Returns the row's number of present slots.
template <bool WITH_ID>
__device__ __forceinline__ int sq_lane_associate(const LaneRows& v, const size_t row, const int N, const int H, const int W,
                                                 const float iou_min, const int* s_bp, const SqBox* s_bbox, unsigned char* match,
                                                 int* fm, unsigned* fid) {
  float bi[SQ_MAXN];
  int bm[SQ_MAXN];
  unsigned bw[SQ_MAXN];
#pragma unroll
  for (int j = 0; j < SQ_MAXN; ++j) { bi[j] = -1.0f; bm[j] = 255; bw[j] = 0u; }
  int n = 0;
  const size_t k0 = sq_lane_slot(v, row, N);
  for (int m = 0; m < N; ++m) {
    if (v.presence[(k0 + m) * v.pres_ld] == 0.0f) continue;
    ++n;
    const SqBox bx = sq_box_of_where(v.where + (k0 + m) * v.where_ld, H, W);
    const unsigned idw = WITH_ID ? sq_word(v.obj_id + (k0 + m) * v.id_ld) : 0u;
#pragma unroll
    for (int j = 0; j < SQ_MAXN; ++j) {
      if (j < N && s_bp[j]) {
        const float iou = sq_box_iou(s_bbox[j], bx);
        if (iou > bi[j]) { bi[j] = iou; bm[j] = m; bw[j] = idw; }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < SQ_MAXN; ++j)
    if (j < N) {
      const bool ok = bi[j] >= iou_min;
      match[j] = (unsigned char)(ok ? bm[j] : 255);
      if (WITH_ID) { fm[j] = ok; fid[j] = ok ? bw[j] : 0u; }
    }
  return n;
}

// Thread c < 4, coordinate c of the boxes staged for the lane's K * S rows q = k * S + s: al = sum of w_k and sum = sum of
// w_k * coordinate over the rows with hit(q), ONE thread's loop over q in index order.
template <class Hit>
__device__ __forceinline__ void sq_lane_box_sum(const float* s_w, const SqBox* s_stage, const int K, const int S, const int c, Hit hit,
                                                float& al, float& sum) {
  al = 0.0f; sum = 0.0f;
  for (int k = 0, q = 0; k < K; ++k) {
    const float w = s_w[k];
    for (int s = 0; s < S; ++s, ++q) {
      if (!hit(q)) continue;
      al += w;
      sum += w * sq_box_coord(s_stage[q], c);
    }
  }
}

// Keep + greedy one-to-one assignment of rows g < G to columns j < N over an IoU table in LDS, iou[g * ld + j] -- ONE thread's walk,
// every array in LDS, nothing indexed in registers.  A pair is eligible when its entry >= iou_min: the caller stores a value below
// every threshold (-1) for a pair that is no candidate, and a NaN never passes.
//   keep   (keep_id != NULL) for g in index order with keep_id[g] >= 0: the first unclaimed j with col_id[j] == keep_id[g] and an
//          eligible entry is matched with g;
//   rest   repeat: the eligible pair of maximal entry among unmatched g and unclaimed j, ties to the smallest g, then the smallest
//          j (a row-major scan with a strict compare); stop when none is left.
// Leaves row_match[g] = j or -1 and col_claim[j] = 1 or 0; returns the number of pairs.  Greedy, not optimal: the
// optimal (Hungarian) assignment is sq_assign_optimal_i32, below, over an int32 table and a whole wavefront's work; the per-frame
// matches of the score, the identity and the trajectory score stay greedy unless sqair_set_lane_match asks for
// sq_assign_keep_optimal, further below; track log scoring (k_lane_tracklog_score) takes its choice of the two as an argument.
__device__ __forceinline__ int sq_assign_keep_greedy(const float* iou, const int ld, const int G, const int N, const float iou_min,
                                                     const int* keep_id, const int* col_id, int* row_match, int* col_claim) {
  int n = 0;
  for (int g = 0; g < G; ++g) row_match[g] = -1;
  for (int j = 0; j < N; ++j) col_claim[j] = 0;
  if (keep_id)
    for (int g = 0; g < G; ++g) {
      const int id = keep_id[g];
      if (id < 0) continue;
      for (int j = 0; j < N; ++j)
        if (!col_claim[j] && col_id[j] == id && iou[g * ld + j] >= iou_min) {
          row_match[g] = j; col_claim[j] = 1; ++n;
          break;
        }
    }
  for (;;) {
    float top = -1.0f;
    int tg = -1, tj = -1;
    for (int g = 0; g < G; ++g) {
      if (row_match[g] >= 0) continue;
      for (int j = 0; j < N; ++j) {
        const float v = iou[g * ld + j];
        if (!col_claim[j] && v >= iou_min && v > top) { top = v; tg = g; tj = j; }
      }
    }
    if (tg < 0) break;
    row_match[tg] = tj; col_claim[tj] = 1; ++n;
  }
  return n;
}

// The column of ONE present lane object j in a table of id words in LDS, cid[0..P) with -1 = free (the IDF's rule 3a, include/sqair_hip.h;
// the HOTA log's too) -- one thread's walk, the objects of a frame in index order, jcol[0..j) holding the columns of the earlier ones
// (any negative value: none).  The column whose word equals `word` is j's, unless an earlier object of the frame holds it; a
// non-negative word that is in no column takes the first free one -- cid is written, `fresh` says so and the caller starts the
// column's other words.  Returns the column, or a negative value for an unkeyed object: a negative word, no free column, a word
// held twice in the frame.
__device__ __forceinline__ int sq_lane_id_column(int* cid, const int P, const int word, const int* jcol, const int j, bool& fresh) {
  fresh = false;
  int col = -1, free_col = -1;
  if (word >= 0) {
    for (int p = 0; p < P; ++p) {
      const int id = cid[p];
      if (id == word) { col = p; break; }
      if (id < 0 && free_col < 0) free_col = p;
    }
    if (col >= 0) {
      for (int jj = 0; jj < j; ++jj)
        if (jcol[jj] == col) col = -2;   // an earlier object of the frame holds the word
    } else if (free_col >= 0) {
      col = free_col;
      cid[col] = word;
      fresh = true;
    }
  }
  return col;
}

// Maximum-weight one-to-one assignment of rows g < G to columns p < P over an int32 table in LDS, w[g * ld + p], for ONE wavefront:
// all 64 lanes call it together, lane p owns column p (P <= 64, G <= 64).  Rows and columns may stay unassigned -- every row g has a
// private dummy column of weight 0, owned by lane g, so a pair of negative weight is never taken --: the optimum is the maximum over
// all partial assignments of the sum of the weights.  Shortest augmenting paths with integer potentials (Hungarian / Jonker-
// Volgenant), rows inserted in index order, O(G^2) wave steps: a step relaxes every unvisited column from the row just reached (one
// column per lane, in registers: the potential, the row assigned to it and that row's potential, the distance, the way back) and
// takes the wave-wide arg-min of the distances, a butterfly of shuffles over (distance, column) keys, ties to the smallest column, the
// real ones before the dummies; then the path is flipped from its free end, one column per step, the owners exchanging rows by
// shuffle.  Nothing is indexed in registers, no barrier is used: the only LDS written is row_to_col, once.  Exact for |weights| below
// 2^30 (the potentials and distances are 64-bit sums of at most G weights; nothing is refused at run time for it).
// Leaves row_to_col[g] = p or -1 (LDS, visible to the wave after the call) and returns the optimum in every lane.
__device__ __forceinline__ long long sq_wave_min_i64(long long v) {
  for (int m = 32; m >= 1; m >>= 1) {
    const long long o = __shfl_xor(v, m, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ long long sq_wave_sum_i64(long long v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ long long sq_assign_optimal_i32(const int* w, const int ld, const int G, const int P, int* row_to_col) {
  constexpr long long FAR = 1ll << 60, NO_KEY = 0x7fffffffffffffffll;
  const int L = threadIdx.x & 63;
  const bool hasA = L < P, hasB = L < G;   // slot A: column L; slot B: the dummy column of row L, number 64 + L
  long long vA = 0, vB = 0, uA = 0, uB = 0;   // the column's potential; the potential of the row assigned to it
  int pA = -1, pB = -1;                        // the row assigned to the column, -1 = free
  for (int i = 0; i < G; ++i) {
    long long dA = FAR, dB = FAR, u_root = 0, u0 = 0;
    bool usedA = !hasA, usedB = !hasB;
    int wayA = -1, wayB = -1, j0 = -1, i0 = i;   // (column -1: the root, row i)
    for (int step = 0; step <= i + 1; ++step) {   // (a path visits at most the i assigned columns and a free one)
      long long key = NO_KEY;
      if (!usedA) {
        const long long cur = -(long long)w[i0 * ld + L] - u0 - vA;
        if (cur < dA) { dA = cur; wayA = j0; }
        key = dA * 256 + L;
      }
      if (!usedB) {
        if (i0 == L && -u0 - vB < dB) { dB = -u0 - vB; wayB = j0; }
        if (dB < FAR) {
          const long long kb = dB * 256 + (64 + L);
          key = kb < key ? kb : key;
        }
      }
      key = sq_wave_min_i64(key);   // (row i's own dummy is free and reachable: there always is one)
      const long long delta = key >> 8;   // (the floor: a distance is negative until the row's potential has absorbed its best weight)
      j0 = (int)(key & 255);
      u_root += delta;
      if (usedA) { uA += delta; vA -= delta; } else if (dA < FAR) dA -= delta;
      if (usedB) { uB += delta; vB -= delta; } else if (dB < FAR) dB -= delta;
      if (j0 == L) usedA = true;
      if (j0 == 64 + L) usedB = true;
      const bool dummy = j0 >= 64;
      i0 = __shfl(dummy ? pB : pA, j0 & 63, 64);
      u0 = __shfl(dummy ? uB : uA, j0 & 63, 64);
      if (i0 < 0) break;   // a free column: the path ends
    }
    for (int step = 0; step <= i + 1; ++step) {   // flip the path: column j0 takes the row of the column before it, the first one the root's
      const bool dummy = j0 >= 64;
      const int j1 = __shfl(dummy ? wayB : wayA, j0 & 63, 64);
      int pr = i;
      long long ur = u_root;
      if (j1 >= 0) {
        const bool d1 = j1 >= 64;
        pr = __shfl(d1 ? pB : pA, j1 & 63, 64);
        ur = __shfl(d1 ? uB : uA, j1 & 63, 64);
      }
      if (j0 == L) { pA = pr; uA = ur; }
      if (j0 == 64 + L) { pB = pr; uB = ur; }
      if (j1 < 0) break;
      j0 = j1;
    }
  }
  if (hasA && pA >= 0) row_to_col[pA] = L;
  if (hasB && pB >= 0) row_to_col[pB] = -1;
  return sq_wave_sum_i64(hasA && pA >= 0 ? (long long)w[pA * ld + L] : 0ll);
}

// Keep + optimal one-to-one assignment (sqair_set_lane_match): sq_assign_keep_greedy's contract -- the same IoU table in LDS, the same
// eligibility (entry >= iou_min; -1 marks a non-candidate; a NaN never passes), the same keep_id / col_id, the same row_match /
// col_claim and return value -- for ONE whole wavefront: all 64 lanes call it together (wave 0 of a 256-thread workgroup -- in
// k_lane_tracklog_score each of the four waves, on tables of its own --; the branch around the call is wave-uniform).  `w` is G * N
// ints of LDS of the caller's, the function's own table.
//   keep   lane 0's walk, exactly the greedy function's keep step: a kept pair is never given up, even where that costs a pair;
//   rest   among the unmatched rows and unclaimed columns the one-to-one assignment of eligible pairs that maximises first the
//          number of pairs, then the sum of q(g, j) = __float2int_rn(iou * 1048576.0f), the IoU in units of 2^-20.  The wave builds
//          the int32 table -- weight 2^25 + q for an eligible pair of an unmatched row and an unclaimed column, -1 for every other
//          pair -- and calls sq_assign_optimal_i32 on it.  An IoU is at most 1, so q <= 2^20; an assignment has at most 16 pairs
//          (G <= 16), so its sum of q is at most 2^24 < 2^25: one pair more outweighs any sum of q, which is cardinality first.
//          Every weight is at most 2^25 + 2^20 < 2^30, the solver's exact range, and a pair of weight -1 is never taken (a row's
//          dummy column weighs 0).  The number of new pairs is the optimum >> 25 for the same reason.
// Among equally optimal assignments the result is whatever sq_assign_optimal_i32 returns: deterministic, not restated as a rule.
// LDS ordering inside the wave: lane 0's keep stores, the table, and the solver's row_to_col are each read by other lanes of the
// same wavefront.  A wavefront's LDS instructions execute in program order, so no wait is needed; sq_wave_lds_order only keeps the
// compiler from moving a lane's loads across another lane's stores (a wavefront-scope fence pair around a wave barrier, neither of
// which is an instruction).  No array is indexed in registers (a lane holds its own row's kept column, one scalar), no scratch, no
// atomics.
__device__ __forceinline__ void sq_wave_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int sq_assign_keep_optimal(const float* iou, const int ld, const int G, const int N, const float iou_min,
                                                      const int* keep_id, const int* col_id, int* row_match, int* col_claim, int* w) {
  const int L = threadIdx.x & 63;
  int n = 0;
  if (L == 0) {
    for (int g = 0; g < G; ++g) row_match[g] = -1;
    for (int j = 0; j < N; ++j) col_claim[j] = 0;
    if (keep_id)
      for (int g = 0; g < G; ++g) {
        const int id = keep_id[g];
        if (id < 0) continue;
        for (int j = 0; j < N; ++j)
          if (!col_claim[j] && col_id[j] == id && iou[g * ld + j] >= iou_min) {
            row_match[g] = j; col_claim[j] = 1; ++n;
            break;
          }
      }
  }
  sq_wave_lds_order();
  const int kept = L < G ? row_match[L] : -1;   // (the solver leaves -1 in the row of a kept pair: every weight of it is -1)
  for (int i = L; i < G * N; i += 64) {
    const int g = i / N, j = i - g * N;
    const float v = iou[g * ld + j];
    w[i] = (row_match[g] < 0 && !col_claim[j] && v >= iou_min) ? (1 << 25) + __float2int_rn(v * 1048576.0f) : -1;
  }
  sq_wave_lds_order();
  const long long opt = sq_assign_optimal_i32(w, N, G, N, row_match);
  sq_wave_lds_order();
  if (L < G) {
    if (kept >= 0) row_match[L] = kept;
    else if (row_match[L] >= 0) col_claim[row_match[L]] = 1;
  }
  sq_wave_lds_order();
  return __shfl(n, 0, 64) + (int)(opt >> 25);
}

// The constant-velocity filter of the motion paragraph (include/sqair_hip.h: sqair_set_motion, points P and U), one (track, axis): k
// points at its five words (p, v, Ppp, Ppv, Pvv).
// P: one frame on; returns S = Ppp' + r.  ONE statement of the step: the identity's motion instantiation calls it on the words in
// LDS, the track log's solve (k_lane_tracklog_smooth) on a thread's own.
__device__ __forceinline__ float sq_kf_predict(float* k, const float q, const float r) {
  const float v = k[1], ppp = k[2], ppv = k[3], pvv = k[4];
  const float npp = ((ppp + 2.0f * ppv) + pvv) + 0.25f * q;
  k[0] = k[0] + v;
  k[2] = npp;
  k[3] = (ppv + pvv) + 0.5f * q;
  k[4] = pvv + q;
  return npp + r;
}
// U: the predicted state with innovation variance S takes the measurement z; returns the posterior velocity.  The solve's: the
// statements of sq_lane_identity_frames<.., true>'s update, restated -- that kernel keeps its own, because calling this function
// from it moved one scalar instruction of its walk, and the identity kernels stay the code they are.  The two
// are held together by bits: tests/test_tracklog_kernel.py compares the solve's velocity with the motion kernel's.
__device__ __forceinline__ float sq_kf_update(float* k, const float S, const float z) {
  const float ppp = k[2], ppv = k[3];
  const float y = z - k[0], k0 = ppp / S, k1 = ppv / S;
  k[0] = fmaf(k0, y, k[0]);
  const float vel = fmaf(k1, y, k[1]);
  k[1] = vel;
  k[2] = (1.0f - k0) * ppp;
  k[3] = (1.0f - k0) * ppv;
  k[4] = fmaf(-k1, ppv, k[4]);
  return vel;
}

// The solve's walk (include/sqair_hip.h: the track log paragraph, points 3 to 5) of ONE (column c, axis ax) of lane b over the window's
// frames: forward -- sq_kf_predict, sq_kf_update on the thread's own five words -- storing state, size and the filtered state; then
// backward (Rauch-Tung-Striebel) over the stepped frames, reading its own stores back.  ONE statement of it: k_lane_tracklog_smooth
// walks its own slots, k_lane_tracklog_stitch the joined ones -- `work` is where the slot of (frame, column) is read, [lag][C] of the
// lane, written by the calling launch in front of a fence and a barrier.  f0..f1 is the column's span (f0 > f1: none: all zeros);
// counts(f) and record(f) are the caller's: whether frame f counts, and its record inside 0..L-1.  A slot read is used inside 0..N-1
// by the caller's construction.  No arrays in registers but a thread's five words, indexed by constants.
template <class Counts, class Record>
__device__ __forceinline__ void sq_tracklog_walk(const SqairTrackLogOut& o, const int* work, const float* lbox, Counts counts, Record record,
                                                 const int f0, const int f1, const int b, const int c, const int ax, const int lag,
                                                 const int B, const int C, const int N, const float q, const float r, const float v0_var) {
  // ---- 3: forward
  float k[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  float size = 0.0f;
  for (int f = 0; f < lag; ++f) {
    const size_t e = ((size_t)f * B + b) * C + c;
    int st = 0;
    if (f >= f0 && f <= f1) {
      if (!counts(f)) {
        st = 3;
      } else {
        const int j = work[f * C + c];
        float z = 0.0f;
        if (j >= 0) {
          const float* w = lbox + ((size_t)record(f) * N + j) * 4;
          size = w[2 + ax];
          z = fmaf(0.5f, size, w[ax]);
        }
        if (f == f0) {
          k[0] = z; k[1] = 0.0f; k[2] = r; k[3] = 0.0f; k[4] = v0_var;
          st = 1;
        } else {
          const float S = sq_kf_predict(k, q, r);
          if (j >= 0) { sq_kf_update(k, S, z); st = 1; }
          else st = 2;
        }
      }
    }
    const bool stepped = st == 1 || st == 2;
    if (ax == 0) o.state[e] = st;
    o.size[e * 2 + ax] = stepped ? size : 0.0f;
    float* w = o.filt + (e * 2 + ax) * 5;
    w[0] = stepped ? k[0] : 0.0f; w[1] = stepped ? k[1] : 0.0f; w[2] = stepped ? k[2] : 0.0f;
    w[3] = stepped ? k[3] : 0.0f; w[4] = stepped ? k[4] : 0.0f;
  }
  // ---- 4: backward over the stepped frames; (ps, vs, as, bs, cs): the smoothed state of the next stepped frame
  float ps = 0.0f, vs = 0.0f, as = 0.0f, bs = 0.0f, cs = 0.0f;
  bool have = false;
  for (int f = lag - 1; f >= 0; --f) {
    const size_t e = (((size_t)f * B + b) * C + c) * 2 + ax;
    float* w = o.smooth + e * 5;
    const bool stepped = f >= f0 && f <= f1 && counts(f);
    if (!stepped) {
      w[0] = 0.0f; w[1] = 0.0f; w[2] = 0.0f; w[3] = 0.0f; w[4] = 0.0f;
      continue;
    }
    const float* fl = o.filt + e * 5;
    const float p = fl[0], v = fl[1], pa = fl[2], pb = fl[3], pc = fl[4];
    if (!have) {
      ps = p; vs = v; as = pa; bs = pb; cs = pc;
      have = true;
    } else {
      float m[5] = {p, v, pa, pb, pc};
      sq_kf_predict(m, q, r);
      const float pm = m[0], am = m[2], bm = m[3], cm = m[4];
      const float det = fmaf(am, cm, -(bm * bm)), m00 = pa + pb, m10 = pb + pc;
      const float g00 = fmaf(m00, cm, -(pb * bm)) / det, g01 = fmaf(pb, am, -(m00 * bm)) / det;
      const float g10 = fmaf(m10, cm, -(pc * bm)) / det, g11 = fmaf(pc, am, -(m10 * bm)) / det;
      const float dp = ps - pm, dv = vs - v, da = as - am, db = bs - bm, dc = cs - cm;
      ps = fmaf(g01, dv, fmaf(g00, dp, p));
      vs = fmaf(g11, dv, fmaf(g10, dp, v));
      const float e00 = fmaf(g01, db, g00 * da), e01 = fmaf(g01, dc, g00 * db);
      const float e10 = fmaf(g11, db, g10 * da), e11 = fmaf(g11, dc, g10 * db);
      as = fmaf(e01, g01, fmaf(e00, g00, pa));
      bs = fmaf(e01, g11, fmaf(e00, g10, pb));
      cs = fmaf(e11, g11, fmaf(e10, g10, pc));
    }
    w[0] = ps; w[1] = vs; w[2] = as; w[3] = bs; w[4] = cs;
  }
}

// The stitch's state distance of one axis (include/sqair_hip.h: the track log stitching paragraph, point 3): `fa` points at the
// predecessor's five filtered words at its last sighting, coasted here `steps` frames with sq_kf_predict; `sb` at the successor's
// five smoothed words at its birth.  Returns d2_axis and leaves det in `det`.  The fma order is the header's.
__device__ __forceinline__ float sq_stitch_d2_axis(const float* fa, const float* sb, const int steps, const float q, const float r, float& det) {
  float k[5] = {fa[0], fa[1], fa[2], fa[3], fa[4]};
  for (int i = 0; i < steps; ++i) sq_kf_predict(k, q, r);
  const float A = k[2] + sb[2], Bm = k[3] + sb[3], Cm = k[4] + sb[4];
  det = fmaf(A, Cm, -(Bm * Bm));
  const float dp = sb[0] - k[0], dv = sb[1] - k[1];
  const float num = fmaf(A * dv, dv, fmaf(-2.0f, Bm * dv, Cm * dp) * dp);
  return num / det;
}
// Both axes of a pair: d2 = d2_y + d2_x; `ok` is the eligibility of point 3 (both det > 0 and d2 <= gate2; a NaN fails).
__device__ __forceinline__ float sq_stitch_d2(const float* fa, const float* sb, const int steps, const float q, const float r,
                                              const float gate2, bool& ok) {
  float det_y, det_x;
  const float d2y = sq_stitch_d2_axis(fa, sb, steps, q, r, det_y);
  const float d2x = sq_stitch_d2_axis(fa + 5, sb + 5, steps, q, r, det_x);
  const float d2 = d2y + d2x;
  ok = det_y > 0.0f && det_x > 0.0f && d2 <= gate2;
  return d2;
}
