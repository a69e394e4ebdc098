// libsqair_hip.so -- the carried model state on the native side of the C ABI (include/sqair_hip.h): the state blob and its
// registration on a handle (sqair_set_state / _smc / _history / _observed), the one resolution of a call (sq_resolve_pass: the
// refusals of a pass, each free of side effects, then the handle's settings by value as an SqStateRes; sq_carry_state: a
// SqairCarry's), the traces of the history ring and the forecast that rolls the prior forward from a state (sqair_forecast), each
// with its lane table.  Host code only; the pass, sq_forward_impl (sqair_api.hip), reads the SqStateRes it is given and nothing
// of the registration; the lane answers a state carries along (estimate, layers, identity, score) are registered and launched in
// sqair_lane_api.hip; the kernels live in sqair_glue.hip and sqair_lane.hip.
#include "sqair_internal.h"
#include "sqair_chain.h"

// carried model state: one blob row per particle row (StateArgs, sqair_glue.h), 4-word aligned
int64_t sq_state_row_floats(const SqairHandle* h) {
  const SqairConfig& c = h->cfg;
  const int64_t N = c.n_steps_per_image, nh = c.n_hidden;
  const int64_t snh = c.time_cell == CELL_LSTM ? 2 * nh : nh, psnh = c.prior_cell == CELL_LSTM ? 2 * nh : nh;
  return (N * (rec::W + snh + psnh) + 2 + 3) / 4 * 4;
}
int sq_state_b_mismatch(SqairHandle* h, const std::string& who, int B) {
  if (B == h->state_B) return 0;
  return sq_no(h, who + "B = " + std::to_string(B) + " but the state set by sqair_set_state is for B = " + std::to_string(h->state_B));
}
static void sq_observed_off(SqairHandle* h) { h->observed = nullptr; h->observed_T = 0; }
static void sq_history_off(SqairHandle* h) { h->hist = SqHistRing{}; h->hist_T = 0; }
extern "C" int64_t sqair_state_bytes(const SqairHandle* h, int B) {
  if (!h || B < 1) return -1;
  return (int64_t)B * h->cfg.k_particles * sq_state_row_floats(h) * 4;
}
extern "C" int sqair_set_state(SqairHandle* h, const void* state_in, void* state_out, const int32_t* src_rows, int64_t state_bytes, int B) {
  if (!h) return -1;
  if (!state_in && !state_out && !src_rows) {
    h->state_on = false; h->state_in = nullptr; h->state_out = nullptr; h->state_src = nullptr; h->state_B = 0;
    h->smc_on = false; h->smc = SqairSmc{};   // (SMC resamples the carried state: off with it)
    sq_history_off(h);                        // (the history records the carried rows: off with it)
    sq_observed_off(h);                       // (the mask is per lane of the carried batch: off with it)
    h->lane = SqLaneSet{};                    // (and so are the lane answers' outputs)
    return 0;
  }
  if (h->cfg.sample_from_prior) return sq_no(h, "sqair_set_state: not with sample_from_prior (generation decides per frame on the host)");
  if (src_rows && !state_in) return sq_no(h, "sqair_set_state: a source map needs state_in");
  if (B < 1 || state_bytes < sqair_state_bytes(h, B))
    return sq_no(h, "sqair_set_state: state_bytes " + std::to_string(state_bytes) + " < sqair_state_bytes(h, " + std::to_string(B) +
                    ") = " + std::to_string(B < 1 ? -1 : sqair_state_bytes(h, B)));
  if (h->smc_on && (!state_in || src_rows != h->state_src || B != h->state_B)) {   // (what SMC was registered against is gone)
    h->smc_on = false; h->smc = SqairSmc{};
  }
  if (h->hist.on && B != h->state_B) sq_history_off(h);   // (the ring was sized for the other B)
  if (B != h->state_B) sq_observed_off(h);                // (and so was the mask)
  if (B != h->state_B) h->lane = SqLaneSet{};             // (and the lane answers' outputs)
  h->state_on = true; h->state_in = state_in; h->state_out = state_out; h->state_src = src_rows; h->state_B = B;
  return 0;
}
// Missing-frame steps (include/sqair_hip.h: sqair_set_observed): the device mask the passes' k_coast_step / k_coast_finish read.
extern "C" int sqair_set_observed(SqairHandle* h, const int32_t* observed, int T, int B) {
  if (!h) return -1;
  if (!observed) {
    sq_observed_off(h);
    return 0;
  }
  if (h->cfg.sample_from_prior) return sq_no(h, "sqair_set_observed: not with sample_from_prior (generation decides per frame on the host)");
  if (!h->state_on) return sq_no(h, "sqair_set_observed: needs a carried state (sqair_set_state): an unobserved lane coasts on the state it carries");
  if (T < 1) return sq_no(h, "sqair_set_observed: T must be >= 1");
  if (sq_state_b_mismatch(h, "sqair_set_observed: ", B) != 0) return -1;
  h->observed = observed; h->observed_T = T;
  return 0;
}
// the refusals of a call while a mask is set (host only: before any HIP call)
int sq_observed_refusal(SqairHandle* h, bool train, int T) {
  if (!h->observed) return 0;
  if (train)
    return sq_no(h, "a mask of observed lanes is set (sqair_set_observed): training on gappy streams is out of scope, switch the mask off "
                    "before a training call");
  if (T != h->observed_T)
    return sq_no(h, "observed (sqair_set_observed): the mask was registered for passes of T = " + std::to_string(h->observed_T) +
                    " frames, a pass of T = " + std::to_string(T) + " cannot read it");
  return 0;
}
// The fields of an SqairSmc that each of its three users checks, -1 + "<who>..." when one is off: ess_frac (in [0, 1]; `train`:
// exactly 1, every lane resampled at every chunk boundary) and the buffers every resampler writes.  `rest`: the caller's own
// further pointers are set too; `names`: how its message lists them all.
static int sq_smc_fields(SqairHandle* h, const std::string& who, const SqairSmc& m, bool train, bool rest, const char* names) {
  if (train && m.ess_frac != 1.0f)
    return sq_no(h, who + "SMC at chunk boundaries needs ess_frac == 1: adaptive resampling (carried weights inside the target) is not "
                          "supported by training");
  if (!(m.ess_frac >= 0.0f && m.ess_frac <= 1.0f)) return sq_no(h, who + "ess_frac must lie in [0, 1]");   // (NaN fails both)
  if (!m.log_w || !m.log_z || !m.log_evidence || !m.ess || !m.resampled || !rest) return sq_no(h, who + names + " must not be NULL");
  return 0;
}
extern "C" int sqair_set_smc(SqairHandle* h, const SqairSmc* smc, int B) {
  if (!h) return -1;
  if (!smc) {
    h->smc_on = false; h->smc = SqairSmc{};
    return 0;
  }
  if (!h->state_on || !h->state_in || !h->state_src)
    return sq_no(h, "sqair_set_smc: needs a carried state with state_in and a source map (sqair_set_state) to resample");
  if (smc->src_rows != h->state_src) return sq_no(h, "sqair_set_smc: src_rows must be the source map given to sqair_set_state");
  if (sq_smc_fields(h, "sqair_set_smc: ", *smc, false, true, "log_w, log_z, log_evidence, ess and resampled") != 0) return -1;
  if (sq_state_b_mismatch(h, "sqair_set_smc: ", B) != 0) return -1;
  h->smc_on = true; h->smc = *smc;
  return 0;
}
// the refusal of a pass with SMC on (host only: before any HIP call)
static int sq_smc_refusal(SqairHandle* h, const SqairOutputs* outp) {
  if (!h->smc_on || (outp && outp->log_weights_per_timestep)) return 0;
  return sq_no(h, "SMC (sqair_set_smc) resamples on log_weights_per_timestep: a pass with SMC on must bind that output");
}
// the resampler's arguments: this pass's log weights `lw` [T][B*K] and row counters `t_row`, the rest from the caller's SqairSmc
SmcArgs sq_smc_args(const SqairSmc& m, const float* lw, const int32_t* t_row, int T, int B, int K) {
  SmcArgs a; memset(&a, 0, sizeof(a));
  a.lw = lw; a.t_row = t_row; a.uniforms = m.uniforms;
  a.log_w = m.log_w; a.log_z = m.log_z; a.log_evidence = m.log_evidence; a.ess = m.ess;
  a.u_out = m.u_out; a.resampled = m.resampled; a.src = m.src_rows;
  a.seed = m.seed; a.ess_frac = m.ess_frac; a.T = T; a.B = B; a.K = K;
  return a;
}
// kernel-level check of the SMC resampler (tests/test_smc_kernel.py): k_smc_resample on caller buffers, K given (1..SQ_MAX_K), no
// state and no pass.  lw [T][B*K]; t_row [B*K] (read only for Philox, when smc->uniforms is NULL); smc->src_rows [B*K] out.
extern "C" int sqair_smc_resample_test(SqairHandle* h, const float* lw, int T, int B, int K, const int32_t* t_row,
                                       const SqairSmc* smc, void* stream) {
  if (!h) return -1;
  if (!lw || !smc || T < 1 || B < 1 || K < 1 || K > SQ_MAX_K || (int64_t)B * K > INT32_MAX)
    return sq_no(h, "sqair_smc_resample_test: null lw / smc or bad T / B / K (1 <= K <= " + std::to_string(SQ_MAX_K) + ")");
  if (sq_smc_fields(h, "sqair_smc_resample_test: ", *smc, false, smc->src_rows && (smc->uniforms || t_row),
                    "log_w, log_z, log_evidence, ess, resampled, src_rows (and t_row without uniforms)") != 0)
    return -1;
  sq_launch_smc_resample(sq_smc_args(*smc, lw, t_row, T, B, K), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// the refusals of a carried training call (host only: before any HIP call)
int sq_carry_refusal(SqairHandle* h, const char* fn, int B, const SqairCarry* carry, const SqairOutputs* out) {
  const std::string f = std::string(fn) + ": ";
  auto no = [&](const std::string& why) { return sq_no(h, f + why); };
  if (!carry) return no("a NULL carry (SqairCarry)");
  if (B != carry->B) return no("B = " + std::to_string(B) + " but the carry is for B = " + std::to_string(carry->B));
  if (B < 1 || carry->state_bytes < sqair_state_bytes(h, B))
    return no("state_bytes " + std::to_string(carry->state_bytes) + " < sqair_state_bytes(h, " + std::to_string(B) + ") = " +
              std::to_string(B < 1 ? -1 : sqair_state_bytes(h, B)));
  if (carry->src_rows && !carry->state_in) return no("a source map needs state_in");
  if (h->state_on) return no("the handle carries an inference state (sqair_set_state): switch it off before training with a carry");
  if (h->cfg.sample_from_prior) return no("a carried state does not combine with sample_from_prior");
  if (!sq_trainable_frame(h)) return -1;
  if (const SqairSmc* m = carry->smc) {
    if (sq_smc_fields(h, f, *m, true, m->src_rows, "the SMC buffers log_w, log_z, log_evidence, ess, resampled and src_rows") != 0)
      return -1;
    if (m->src_rows != carry->src_rows) return no("smc->src_rows must be the carry's src_rows");
    if (out && !out->log_weights_per_timestep)
      return no("SMC resamples on log_weights_per_timestep: a carried step with SMC must bind that output");
  }
  return 0;
}
// the refusals of a pass with a carried state (host only: before any HIP call)
int sq_state_refusal(SqairHandle* h, bool train, int B, int t_offset) {
  if (!h->state_on) return 0;
  if (train) return sq_no(h, "a carried state (sqair_set_state) is for inference passes: training / backward with one is not supported");
  if (h->cfg.sample_from_prior) return sq_no(h, "a carried state (sqair_set_state) does not combine with sample_from_prior");
  if (h->state_in && t_offset != 0)
    return sq_no(h, "with state_in set (sqair_set_state) t_offset must be 0: the state's frame counter is the time index");
  return sq_state_b_mismatch(h, "", B);
}

SqStateRes sq_carry_state(const SqairCarry* c) {
  SqStateRes st;
  st.on = true; st.in = c->state_in; st.out = c->state_out; st.src = c->src_rows;
  st.fresh = true;
  if (c->smc) { st.smc_on = true; st.smc = *c->smc; }
  return st;
}
// k_state_import's / k_state_export's arguments: the frame's records, states, last ids and row counters `t_row` (and, for the
// import of a training pass, its fresh / imported flags, else NULL) against the blobs and source map of `st`
StateArgs sq_state_args(const SqairHandle* h, const SqStateRes& st, int R, float* rec, float* temporal, float* prior, float* last_id,
                        int* t_row, float* fresh, int t0) {
  const Dims d = make_dims(h->cfg, 1);
  StateArgs a; memset(&a, 0, sizeof(a));
  a.rec = rec; a.temporal = temporal; a.prior = prior; a.last_id = last_id; a.t_row = t_row; a.fresh = fresh;
  a.blob_in = (const float*)st.in;
  a.blob_out = (float*)st.out;
  a.src = st.src;
  a.R = R; a.n_rec = d.N * rec::W; a.n_tmp = d.N * d.snh; a.n_pri = d.N * d.psnh; a.row_words = (int)sq_state_row_floats(h);
  a.t0 = t0;
  return a;
}

// ------------------------------------------------------------------------------------------------
// track history (include/sqair_hip.h: sqair_set_history / sqair_history_trace): the ring's layout, registration and refusals, the
// argument blocks of k_history_push (launched by sq_forward_impl) and of the trace kernels
// ------------------------------------------------------------------------------------------------
static HistLayout sq_hist_layout(const SqairHandle* h, int L, int T, int B, uint32_t fields) {
  const SqairConfig& c = h->cfg;
  HistLayout y; memset(&y, 0, sizeof(y));
  y.L = L; y.T = T; y.K = c.k_particles; y.R = B * c.k_particles; y.N = c.n_steps_per_image; y.nw = c.n_what; y.fields = fields;
  const long long R = y.R, TRN = (long long)T * R * y.N;
  y.o_where = 2 * R;   // (parent at 0, t0 at R)
  y.o_pres = y.o_where + TRN * 4;
  y.o_id = y.o_pres + TRN;
  y.o_what = y.o_id + TRN;
  y.o_lw = y.o_what + ((fields & SQAIR_HIST_WHAT) ? TRN * y.nw : 0);
  y.slot_words = align64(y.o_lw + ((fields & SQAIR_HIST_LOG_W) ? (long long)T * R : 0));
  y.scratch = SQ_HIST_HDR;
  y.slots = align64(y.scratch + (long long)L * R);
  y.total = y.slots + (long long)L * y.slot_words;
  return y;
}
static bool sq_hist_fields_ok(uint32_t fields) {
  return (fields & SQAIR_HIST_MANDATORY) == SQAIR_HIST_MANDATORY && (fields & ~SQAIR_HIST_ALL) == 0;
}
extern "C" int64_t sqair_history_bytes(const SqairHandle* h, int L, int T, int B, uint32_t fields) {
  if (!h || L < 1 || T < 1 || B < 1 || !sq_hist_fields_ok(fields) || (int64_t)B * h->cfg.k_particles > INT32_MAX) return -1;
  return sq_hist_layout(h, L, T, B, fields).total * 4;
}
extern "C" int sqair_set_history(SqairHandle* h, void* ring, int64_t ring_bytes, int L, uint32_t fields) {
  if (!h) return -1;
  if (!ring) {
    sq_history_off(h);
    return 0;
  }
  if (!h->state_on) return sq_no(h, "sqair_set_history: needs a carried state (sqair_set_state): the history records the rows it carries");
  if (L < 1) return sq_no(h, "sqair_set_history: L must be >= 1");
  if (!sq_hist_fields_ok(fields))
    return sq_no(h, "sqair_set_history: fields must hold where, presence and obj_id (SQAIR_HIST_MANDATORY) and no bit outside SQAIR_HIST_ALL");
  const int64_t need = sqair_history_bytes(h, L, 1, h->state_B, fields);
  if (ring_bytes < need)
    return sq_no(h, "sqair_set_history: ring_bytes " + std::to_string(ring_bytes) + " < sqair_history_bytes(h, " + std::to_string(L) +
                    ", 1, " + std::to_string(h->state_B) + ", fields) = " + std::to_string(need));
  h->hist.on = true; h->hist.ring = ring; h->hist.bytes = ring_bytes; h->hist.L = L; h->hist_T = 0; h->hist.fields = fields;
  return 0;
}
// the refusal of a pass with history on (host only: before any HIP call; sq_resolve_pass fixes the ring's T)
static int sq_history_refusal(SqairHandle* h, int T, int B, const SqairOutputs* outp) {
  if (!h->state_on || !h->hist.on) return 0;
  if (T < 1 || B != h->state_B) return 0;   // (the pass's own checks refuse these)
  if (h->hist_T != 0 && T != h->hist_T)
    return sq_no(h, "history (sqair_set_history): this ring's slots hold passes of T = " + std::to_string(h->hist_T) + " frames, a pass of T = " +
                    std::to_string(T) + " cannot be pushed into it");
  const int64_t need = sqair_history_bytes(h, h->hist.L, T, B, h->hist.fields);
  if (h->hist.bytes < need)
    return sq_no(h, "history (sqair_set_history): ring_bytes " + std::to_string(h->hist.bytes) + " < sqair_history_bytes(h, " +
                    std::to_string(h->hist.L) + ", " + std::to_string(T) + ", " + std::to_string(B) + ", fields) = " + std::to_string(need));
  const uint32_t f = h->hist.fields;
  if (!outp || !outp->where || !outp->presence || !outp->obj_id || ((f & SQAIR_HIST_WHAT) && !outp->what) ||
      ((f & SQAIR_HIST_LOG_W) && !outp->log_weights_per_timestep))
    return sq_no(h, "history (sqair_set_history) records the pass's outputs: a pass with history on must bind where, presence, obj_id and "
                    "the optional fields it was set with (what, log_weights_per_timestep)");
  return 0;
}
int sq_resolve_pass(SqairHandle* h, bool train, int T, int B, int t_offset, const SqairOutputs* out, SqStateRes* st) {
  if (sq_observed_refusal(h, train, T) != 0 || sq_state_refusal(h, train, B, t_offset) != 0 || sq_smc_refusal(h, out) != 0 ||
      sq_history_refusal(h, T, B, out) != 0 || sq_estimate_refusal(h, T, out) != 0)
    return -1;
  SqStateRes r;
  r.on = h->state_on; r.in = h->state_in; r.out = h->state_out; r.src = h->state_src;
  r.smc_on = h->smc_on; r.smc = h->smc;
  if (r.on) {   // (what rides on the carried state: all off without one)
    r.observed = h->observed; r.hist = h->hist; r.lane = h->lane;
    r.lane.score_match = h->match_score; r.lane.ident_match = h->match_ident;   // (sqair_set_lane_match: read here, at launch time)
  }
  *st = r;
  if (r.hist.on && T >= 1) h->hist_T = T;   // (T < 1 is the pass's own to refuse)
  return 0;
}
SqStateRes sq_without_effects(SqStateRes st) {
  st.out = nullptr; st.smc_on = false; st.smc = SqairSmc{};
  st.hist = SqHistRing{};
  st.lane = SqLaneSet{};
  return st;
}
HistPushArgs sq_history_push_args(const SqairHandle* h, const SqStateRes& st, const SqairOutputs& out, const int* t_row, int T, int B) {
  HistPushArgs a; memset(&a, 0, sizeof(a));
  a.ring = (unsigned*)st.hist.ring;
  a.lay = sq_hist_layout(h, st.hist.L, T, B, st.hist.fields);
  a.where = out.where; a.presence = out.presence; a.obj_id = out.obj_id; a.what = out.what; a.lw = out.log_weights_per_timestep;
  a.src = st.src; a.have_in = st.in != nullptr; a.t_row = t_row;
  return a;
}
// the refusals of a trace and its argument block (host only): sqair_history_trace and sqair_history_trace_lane, one body
static int sq_history_trace_args(SqairHandle* h, const std::string& who, void* ring, const int32_t* src_next, int lag,
                                 const SqairTraceOutputs* outp, HistTraceArgs& a) {
  if (!h->state_on || !h->hist.on) return sq_no(h, who + "no history set (sqair_set_history)");
  if (!ring || ring != h->hist.ring) return sq_no(h, who + "ring must be the ring given to sqair_set_history");
  if (lag < 1 || lag > h->hist.L)
    return sq_no(h, who + "lag = " + std::to_string(lag) + " must lie in [1, L = " + std::to_string(h->hist.L) + "]");
  if (!outp) return sq_no(h, who + "out must not be NULL");
  const SqairTraceOutputs& o = *outp;
  if (o.T < 1) return sq_no(h, who + "out->T (frames per pass) must be >= 1");
  if (h->hist_T != 0 && o.T != h->hist_T)
    return sq_no(h, who + "out->T = " + std::to_string(o.T) + " but the passes pushed have T = " + std::to_string(h->hist_T));
  if (h->hist.bytes < sqair_history_bytes(h, h->hist.L, o.T, h->state_B, h->hist.fields))
    return sq_no(h, who + "the ring is too small for passes of out->T = " + std::to_string(o.T) + " frames");
  if ((o.what && !(h->hist.fields & SQAIR_HIST_WHAT)) || (o.log_w && !(h->hist.fields & SQAIR_HIST_LOG_W)))
    return sq_no(h, who + "what / log_w asked of a ring that was set without the field");
  const bool table = o.track_id || o.n_tracks || o.track_present || o.track_where;
  if (table && (o.max_tracks < 1 || o.max_tracks > SQ_HIST_MAX_TRACKS))
    return sq_no(h, who + "max_tracks must lie in [1, " + std::to_string(SQ_HIST_MAX_TRACKS) + "] for the track table");
  memset(&a, 0, sizeof(a));
  a.ring = (unsigned*)ring;
  a.lay = sq_hist_layout(h, h->hist.L, o.T, h->state_B, h->hist.fields);
  if ((int64_t)a.lay.R * lag > INT32_MAX || (int64_t)lag * o.T * a.lay.N * (table ? o.max_tracks : 1) > INT32_MAX)
    return sq_no(h, who + "lag * rows (or lag * T * N * max_tracks) beyond 2^31");
  a.src_next = src_next; a.lag = lag; a.M = table ? o.max_tracks : 1;
  a.where = o.where; a.presence = o.presence; a.obj_id = o.obj_id; a.what = o.what; a.log_w = o.log_w;
  a.valid = o.valid; a.frame_index = o.frame_index; a.ancestor_row = o.ancestor_row; a.unique_ancestors = o.unique_ancestors;
  a.track_id = o.track_id; a.n_tracks = o.n_tracks; a.track_present = o.track_present; a.track_where = o.track_where;
  return 0;
}
extern "C" int sqair_history_trace(SqairHandle* h, void* ring, const int32_t* src_next, int lag, const SqairTraceOutputs* outp,
                                   void* stream) {
  if (!h) return -1;
  HistTraceArgs a;
  if (sq_history_trace_args(h, "sqair_history_trace: ", ring, src_next, lag, outp, a) != 0) return -1;
  sq_launch_history_trace(a, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------
// lane tracks (include/sqair_hip.h: sqair_history_trace_lane): the trace, then the lane forecast's kernels run backwards over the
// traced rows (TrackLaneArgs)
// ------------------------------------------------------------------------------------------------
extern "C" int64_t sqair_trace_lane_scratch_bytes(const SqairHandle* h, int B, int K) {
  return sqair_forecast_lane_scratch_bytes(h, B, K);   // (the same weights, association and followed ids between the two launches)
}
static int sq_trace_lane_fields(SqairHandle* h, const std::string& who, const SqairTraceLane* l, int F, int B, int K, const void* scratch,
                                int64_t scratch_bytes) {
  if (!l) return sq_no(h, who + "lane must not be NULL");
  if (sq_unit_refusal(h, who, "lane->iou_min", l->iou_min) != 0) return -1;
  if (!l->best_row) return sq_no(h, who + "lane->best_row must not be NULL");
  if (K > SQ_MAX_K) return sq_no(h, who + "K = " + std::to_string(K) + " particles per lane, above " + std::to_string(SQ_MAX_K));
  if (F > 65535) return sq_no(h, who + "F = " + std::to_string(F) + " traced frames, above 65535");
  const int64_t need = sqair_trace_lane_scratch_bytes(h, B, K);
  if (!scratch || scratch_bytes < need)
    return sq_no(h, who + "scratch is NULL or scratch_bytes " + std::to_string(scratch_bytes) + " < sqair_trace_lane_scratch_bytes(h, " +
                    std::to_string(B) + ", " + std::to_string(K) + ") = " + std::to_string(need));
  return 0;
}
static TrackLaneArgs sq_track_lane_args(const SqairHandle* h, const float* where, const float* presence, const float* obj_id,
                                        const int32_t* valid, const float* log_w, int F, int B, int K, const SqairTraceLane& l,
                                        void* scratch) {
  const SqairConfig& c = h->cfg;
  const int N = c.n_steps_per_image;
  const size_t last = (size_t)(F - 1) * B * K * N;   // slot 0 of row 0 of the newest frame
  TrackLaneArgs a; memset(&a, 0, sizeof(a));
  ForecastLaneArgs& g = a.f;
  g.start = LaneRows{where + last * 4, 4, presence + last, 1, obj_id + last, 1, 1};
  g.where = where; g.where_ld = 4; g.presence = presence; g.pres_ld = 1; g.obj_id = obj_id; g.id_ld = 1;
  g.log_w = log_w; g.x = sq_forecast_lane_scratch((float*)scratch, B, K, N);
  g.lane.iou_min = l.iou_min; g.lane.best_row = l.best_row; g.lane.weights = l.weights; g.lane.obj_id = l.obj_id;
  g.lane.presence = l.presence; g.lane.box0 = l.box0; g.lane.support = l.support; g.lane.alive = l.alive; g.lane.box_mean = l.box_mean;
  g.lane.box_std = l.box_std; g.lane.count_prob = l.count_prob;
  g.F = F; g.B = B; g.K = K; g.S = 1; g.N = N; g.H = c.img_h; g.W = c.img_w;
  a.valid = valid; a.first_frame = l.first_frame; a.valid_mass = l.valid_mass;
  return a;
}
extern "C" int sqair_history_trace_lane(SqairHandle* h, void* ring, const int32_t* src_next, int lag, const SqairTraceOutputs* outp,
                                        const float* log_w, const SqairTraceLane* lane, void* scratch, int64_t scratch_bytes,
                                        void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_history_trace_lane: ";
  HistTraceArgs a;
  if (sq_history_trace_args(h, who, ring, src_next, lag, outp, a) != 0) return -1;
  const int F = lag * outp->T, B = h->state_B, K = h->cfg.k_particles;
  if (sq_trace_lane_fields(h, who, lane, F, B, K, scratch, scratch_bytes) != 0) return -1;
  if (!outp->where || !outp->presence || !outp->obj_id || !outp->valid)
    return sq_no(h, who + "the lane kernels read the gathered rows: out->where, out->presence, out->obj_id and out->valid must be bound");
  sq_launch_history_trace(a, (hipStream_t)stream);
  sq_launch_track_lane(sq_track_lane_args(h, outp->where, outp->presence, outp->obj_id, outp->valid, log_w, F, B, K, *lane, scratch),
                       (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// kernel-level check of the lane tracks (tests/test_track_lane_kernel.py): the two kernels on caller tensors, K given, no ring
extern "C" int sqair_track_lane_test(SqairHandle* h, const float* where, const float* presence, const float* obj_id, const int32_t* valid,
                                     const float* log_w, int F, int B, int K, const SqairTraceLane* lane, void* scratch,
                                     int64_t scratch_bytes, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_track_lane_test: ";
  if (!where || !presence || !obj_id || !valid || !lane || !scratch)
    return sq_no(h, who + "null where / presence / obj_id / valid / lane / scratch");
  if (F < 1 || F > 65535 || B < 1 || K < 1 || K > SQ_MAX_K || (int64_t)F * B * K * h->cfg.n_steps_per_image > INT32_MAX)
    return sq_no(h, who + "bad F / B / K (1 <= F <= 65535, 1 <= K <= " + std::to_string(SQ_MAX_K) + ", F * B * K * N within int32)");
  if (sq_trace_lane_fields(h, who, lane, F, B, K, scratch, scratch_bytes) != 0) return -1;
  sq_launch_track_lane(sq_track_lane_args(h, where, presence, obj_id, valid, log_w, F, B, K, *lane, scratch), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------------------------------------
// forecast (include/sqair_hip.h: sqair_forecast): the propagation prior rolled F frames forward from the carried state, discovery
// empty, then the decoder of all F frames and the predictive summaries
// ------------------------------------------------------------------------------------------------
struct FcWorkspace {
  float* rec;        // [F + 1][M][rec::W]: frame 0 = the imported state, frame f + 1 = forecast frame f
  float* temporal;   // [M][snh] (written by the import, never read)
  float* prior[2];   // [M][psnh] compacted prior states, ping-pong over frames
  float* prior_p;    // [M][psnh] the prior cell's output of the frame
  float *pgz, *pgrh, *pgxh;   // prior cell internals (GRU: z gate, r h, x h; LSTM: pgz = the four gate pre-activations)
  float* pstats;     // [M][PS_LD]
  float* last_id;    // [R]
  int* t_row;        // [R]
  float *disc_init_rec, *prop_rnn_init, *disc_rnn_init, *rn_init_state, *w3_prop, *w3_disc;   // (k_init_state writes them)
  float *dec_a, *dec_b, *glimpse;   // decoder of all F frames [F * M][nh | G*G]
  float* canvas;     // [F][R][H*W] when the caller asks for summaries but not for the canvas
  int64_t total;     // floats
};
static FcWorkspace fc_carve(const SqairHandle* h, int F, int B, float* base) {
  const SqairConfig& c = h->cfg;
  const int64_t nh = c.n_hidden, N = c.n_steps_per_image, R = (int64_t)B * c.k_particles, M = R * N;
  const int64_t snh = c.time_cell == CELL_LSTM ? 2 * nh : nh, psnh = c.prior_cell == CELL_LSTM ? 2 * nh : nh;
  FcWorkspace w;
  memset(&w, 0, sizeof(w));
  int64_t o = 0;
  auto take = [&](int64_t n) {
    float* p = base ? base + o : nullptr;
    o += align64(n);
    return p;
  };
  w.rec = take((int64_t)(F + 1) * M * rec::W);
  w.temporal = take(M * snh);
  w.prior[0] = take(M * psnh);
  w.prior[1] = take(M * psnh);
  w.prior_p = take(M * psnh);
  w.pgz = take(M * (c.prior_cell == CELL_LSTM ? 4 * nh : nh));
  w.pgrh = take(M * nh);
  w.pgxh = take(M * nh);
  w.pstats = take(M * PS_LD);
  w.last_id = take(R);
  w.t_row = (int*)take(R);
  w.disc_init_rec = take(rec::W);
  w.prop_rnn_init = take(2 * nh);
  w.disc_rnn_init = take(2 * nh);
  w.rn_init_state = take(4);
  w.w3_prop = take(nh * 8 + 8);
  w.w3_disc = take(nh * 8 + 8);
  w.dec_a = take((int64_t)F * M * nh);
  w.dec_b = take((int64_t)F * M * nh);
  w.glimpse = take((int64_t)F * M * c.glimpse_size * c.glimpse_size);
  w.canvas = take((int64_t)F * R * c.img_h * c.img_w);
  w.total = o;
  return w;
}
extern "C" int64_t sqair_forecast_workspace_bytes(const SqairHandle* h, int F, int B) {
  if (!h || F < 1 || B < 1) return -1;
  return fc_carve(h, F, B, nullptr).total * 4;
}
// The fan-out's workspace: the forecast's own for B * S lanes' worth of rows (the per-row kernels never look at lane structure),
// then the expanded source map [R*S] and the lane forecast's scratch.
static bool fc_fan_fits(const SqairHandle* h, int B, int S) {
  return S >= 1 && (int64_t)h->cfg.k_particles * S <= SQAIR_FORECAST_FAN_MAX &&
         (int64_t)B * h->cfg.k_particles * S * h->cfg.n_steps_per_image <= INT32_MAX;
}
extern "C" int64_t sqair_forecast_fan_workspace_bytes(const SqairHandle* h, int F, int B, int S) {
  if (!h || F < 1 || B < 1 || !fc_fan_fits(h, B, S)) return -1;
  const int64_t K = h->cfg.k_particles, N = h->cfg.n_steps_per_image;
  return (fc_carve(h, F, B * S, nullptr).total + align64((int64_t)B * K * S) + sq_forecast_lane_scratch_words(B, K, N)) * 4;
}
extern "C" int64_t sqair_forecast_lane_scratch_bytes(const SqairHandle* h, int B, int K) {
  if (!h || B < 1 || K < 1 || K > SQ_MAX_K) return -1;
  return sq_forecast_lane_scratch_words(B, K, h->cfg.n_steps_per_image) * 4;
}
static int sq_forecast_lane_fields(SqairHandle* h, const std::string& who, const SqairForecastLane& l) {
  if (sq_unit_refusal(h, who, "lane->iou_min", l.iou_min) != 0) return -1;
  if (!l.best_row) return sq_no(h, who + "lane->best_row must not be NULL");
  return 0;
}
// sqair_forecast (fan = false: S = 1, no lane, its own workspace size) and sqair_forecast_fan: one body
static int sq_forecast_impl(SqairHandle* h, const bool fan, const float* flat_params, const void* packed_v, const float* noise, int F,
                            int B, int S, const int32_t* src_rows, const SqairForecastOutputs* outp, const SqairForecastLane* lane,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  if (!h) return -1;
  const SqairConfig& c = h->cfg;
  const std::string fn = fan ? "sqair_forecast_fan" : "sqair_forecast", who = fn + ": ";
  if (c.sample_from_prior) return sq_no(h, who + "not with sample_from_prior (the forecast is the generation mode, from a carried state)");
  if (!h->state_on || !h->state_in) return sq_no(h, who + "needs a carried state with state_in (sqair_set_state) to start from");
  if (sq_state_b_mismatch(h, who, B) != 0) return -1;
  if (F < 1) return sq_no(h, who + "F must be >= 1");
  if (!noise) return sq_no(h, who + "noise must not be NULL");
  if (!flat_params || !packed_v || !outp || !workspace) return sq_no(h, who + "null parameters, packed buffer, outputs or workspace");
  if (fan) {
    if (S < 1) return sq_no(h, who + "S must be >= 1");
    if ((int64_t)c.k_particles * S > SQAIR_FORECAST_FAN_MAX)
      return sq_no(h, who + "K * S = " + std::to_string((int64_t)c.k_particles * S) + " rollouts per lane, above SQAIR_FORECAST_FAN_MAX = " +
                      std::to_string(SQAIR_FORECAST_FAN_MAX));
    if (!fc_fan_fits(h, B, S)) return sq_no(h, who + "B * K * S * N slots do not fit int32");
  }
  const int64_t need = fan ? sqair_forecast_fan_workspace_bytes(h, F, B, S) : sqair_forecast_workspace_bytes(h, F, B);
  if (workspace_bytes < need)
    return sq_no(h, who + "workspace_bytes " + std::to_string(workspace_bytes) + " < " + fn + "_workspace_bytes(h, " +
                    std::to_string(F) + ", " + std::to_string(B) + (fan ? ", " + std::to_string(S) : std::string()) + ") = " + std::to_string(need));
  if (lane) {
    if (sq_forecast_lane_fields(h, who, *lane) != 0) return -1;
    if (F > 65535) return sq_no(h, who + "with lane set F must be <= 65535");
  }
  const float* packed = (const float*)packed_v;
  const float* flat = sq_flat(h, flat_params, packed);
  sq_chain_reset(h);
  hipStream_t s = (hipStream_t)stream;
  const SqairForecastOutputs out = *outp;
  // R: the rollout rows, q = r * S + s -- B * S lanes' worth of rows to every per-row kernel; only the import map, the summaries
  // and the lane forecast know the lanes
  const int nh = c.n_hidden, N = c.n_steps_per_image, K = c.k_particles, R = B * S * K, M = R * N, RW = rec::W;
  const int G2 = c.glimpse_size * c.glimpse_size;
  const Dims d = make_dims(c, B * S);
  const int psnh = d.psnh;
  const POff po = h->po;
  const FcWorkspace w = fc_carve(h, F, B * S, (float*)workspace);
  int* src_fan = (int*)((float*)workspace + w.total);                                  // [R] (fan only)
  float* lane_scratch = (float*)workspace + w.total + align64((int64_t)R);             // (fan only)
  // prologue: the rows the next pass would start from (the pass's own k_init_state + k_state_import, into this workspace)
  sq_launch_init_state(w.rec, w.temporal, w.prior[0], w.last_id, w.disc_init_rec, w.prop_rnn_init, w.disc_rnn_init, w.rn_init_state,
                       w.w3_prop, w.w3_disc, (int)P(h, "prop.transform.l2.w"), (int)P(h, "disc.transform.l2.w"), flat, po, d, s);
  const int32_t* src = src_rows ? src_rows : h->state_src;
  if (S > 1) {   // (the map fanned out into the workspace; k_state_import then bounds it against R, which its -1s pass)
    sq_launch_forecast_fan_src(src, src_fan, B * K, S, s);
    src = src_fan;
  }
  SqStateRes st;   // (an import only: nothing exported, pushed or resampled)
  st.on = true; st.in = h->state_in; st.src = src;
  sq_launch_state_import(sq_state_args(h, st, R, w.rec, w.temporal, w.prior[0], w.last_id, w.t_row, nullptr, 0), s);
  // per frame: the prior cell over all M slots (section A of the pass), then sampling + ids + compaction in one launch
  for (int f = 0; f < F; ++f) {
    const float* rec_prev = w.rec + (size_t)f * M * RW;
    const float* prior_prev = w.prior[f & 1];
    const int rc = sq_prior_step(h, packed, s, M, rec_prev, prior_prev, w.prior_p, w.pgz, w.pgrh, w.pgxh, w.pstats, nullptr, nullptr);
    if (rc != 0) return rc;
    ForecastArgs fa; memset(&fa, 0, sizeof(fa));
    fa.rec_prev = rec_prev; fa.pstats = w.pstats; fa.ps_ld = PS_LD; fa.prior_p = w.prior_p;
    fa.noise = noise + (size_t)f * R * 2 * N * d.nzw; fa.rec_next = w.rec + (size_t)(f + 1) * M * RW; fa.prior_next = w.prior[(f + 1) & 1];
    fa.f = f; fa.out = out; fa.cfg = c;
    sq_launch_forecast_step(fa, d, s);
  }
  const float* rec_all = w.rec + (size_t)M * RW;
  if (lane) {   // the lane forecast needs only the records: frame 0 = the start rows (S copies of each), frames 1..F the rollouts
    ForecastLaneArgs la; memset(&la, 0, sizeof(la));
    la.start = LaneRows{w.rec + rec::WHERE, RW, w.rec + rec::PRES, RW, w.rec + rec::ID, RW, S};
    la.where = rec_all + rec::WHERE; la.presence = rec_all + rec::PRES; la.obj_id = rec_all + rec::ID;
    la.where_ld = la.pres_ld = la.id_ld = RW;
    la.log_w = out.log_w; la.x = sq_forecast_lane_scratch(lane_scratch, B, K, N); la.lane = *lane;
    la.F = F; la.B = B; la.K = K; la.S = S; la.N = N; la.H = c.img_h; la.W = c.img_w;
    sq_launch_forecast_lane(la, s);
  }
  // decoder of all F frames (section J of the pass without the likelihood): three M = F*B'*N row GEMMs + the canvas-only insert
  float* canvas = out.canvas ? out.canvas : w.canvas;
  const bool want_canvas = out.canvas || out.mean_canvas;
  if (want_canvas || out.glimpse) {
    const int MT = F * M;
    float* gl = out.glimpse ? out.glimpse : w.glimpse;
    Lin a; a.seg(rec_all, RW, rec::ZW).out(w.dec_a, nh).act(ACT_ELU); RUN(a, L_DEC0, MT);
    Lin b; b.seg(w.dec_a, nh, nh).out(w.dec_b, nh).act(ACT_ELU); RUN(b, L_DEC1, MT);
    Lin g; g.seg(w.dec_b, nh, nh).out(gl, G2); g.a.scale_ptr = flat + po.dec_output_scale; RUN(g, L_DEC2, MT);
    if (want_canvas) {
      InsertArgs ia; memset(&ia, 0, sizeof(ia));
      ia.glimpse = gl; ia.rec = rec_all; ia.rec_ld = RW; ia.mean_img = flat + po.dec_mean_img; ia.canvas = canvas; ia.n_frames = F;
      ia.std_fg = c.output_std; ia.std_bg = c.background_std;
      if (sq_launch_insert_canvas(ia, d, s) != 0) { sq_set_error(h, "sqair_forecast: the decoder canvas launch failed (dynamic LDS limit)"); return -2; }
    }
  }
  if (out.mean_canvas || out.expected_count) {
    ForecastSummaryArgs sa; memset(&sa, 0, sizeof(sa));
    sa.canvas = canvas; sa.rec = rec_all; sa.log_w = out.log_w; sa.mean_canvas = out.mean_canvas; sa.expected_count = out.expected_count;
    sa.F = F; sa.B = B; sa.K = K; sa.S = S; sa.N = N; sa.P = c.img_h * c.img_w;
    sq_launch_forecast_summary(sa, s);
  }
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int sqair_forecast(SqairHandle* h, const float* flat_params, const void* packed_v, const float* noise, int F, int B,
                              const int32_t* src_rows, const SqairForecastOutputs* outp, void* workspace, int64_t workspace_bytes,
                              void* stream) {
  return sq_forecast_impl(h, false, flat_params, packed_v, noise, F, B, 1, src_rows, outp, nullptr, workspace, workspace_bytes, stream);
}
extern "C" int sqair_forecast_fan(SqairHandle* h, const float* flat_params, const void* packed_v, const float* noise, int F, int B, int S,
                                  const int32_t* src_rows, const SqairForecastOutputs* outp, const SqairForecastLane* lane,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  return sq_forecast_impl(h, true, flat_params, packed_v, noise, F, B, S, src_rows, outp, lane, workspace, workspace_bytes, stream);
}
// kernel-level check of the lane forecast (tests/test_forecast_lane_kernel.py): the two kernels on caller tensors, K and S given
extern "C" int sqair_forecast_lane_test(SqairHandle* h, const float* start_where, const float* start_presence, const float* start_obj_id,
                                        const float* where, const float* presence, const float* obj_id, const float* log_w, int F, int B,
                                        int K, int S, const SqairForecastLane* lane, void* scratch, int64_t scratch_bytes, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_forecast_lane_test: ";
  const SqairConfig& c = h->cfg;
  if (!start_where || !start_presence || !start_obj_id || !where || !presence || !obj_id || !lane || !scratch)
    return sq_no(h, who + "null start_where / start_presence / start_obj_id / where / presence / obj_id / lane / scratch");
  if (F < 1 || F > 65535 || B < 1 || K < 1 || K > SQ_MAX_K || S < 1 || (int64_t)K * S > SQAIR_FORECAST_FAN_MAX ||
      (int64_t)B * K * S * c.n_steps_per_image > INT32_MAX)
    return sq_no(h, who + "bad F / B / K / S (1 <= K <= " + std::to_string(SQ_MAX_K) + ", K * S <= " + std::to_string(SQAIR_FORECAST_FAN_MAX) + ")");
  if (sq_forecast_lane_fields(h, who, *lane) != 0) return -1;
  if (scratch_bytes < sqair_forecast_lane_scratch_bytes(h, B, K))
    return sq_no(h, who + "scratch_bytes " + std::to_string(scratch_bytes) + " < sqair_forecast_lane_scratch_bytes(h, " + std::to_string(B) +
                    ", " + std::to_string(K) + ") = " + std::to_string(sqair_forecast_lane_scratch_bytes(h, B, K)));
  ForecastLaneArgs la; memset(&la, 0, sizeof(la));
  la.start = LaneRows{start_where, 4, start_presence, 1, start_obj_id, 1, 1};
  la.where = where; la.where_ld = 4; la.presence = presence; la.pres_ld = 1; la.obj_id = obj_id; la.id_ld = 1;
  la.log_w = log_w; la.x = sq_forecast_lane_scratch((float*)scratch, B, K, c.n_steps_per_image); la.lane = *lane;
  la.F = F; la.B = B; la.K = K; la.S = S; la.N = c.n_steps_per_image; la.H = c.img_h; la.W = c.img_w;
  sq_launch_forecast_lane(la, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
