// libsqair_hip.so -- the lane answers on the native side of the C ABI (include/sqair_hip.h): the estimate and its followers, the
// layers, the identity, the track log, the score, the IDF1 table and the HOTA log.  Their registration on a handle as one block (SqLaneSet, sqair_internal.h:
// sqair_set_estimate / _layers / _score / _identity / _motion / _tracklog / _score_ids / _idf / _hota), the estimate's refusal of a pass, ONE builder per kernel's arguments -- called by the
// pass and by the kernel-level entry point alike --, the pass's launch sequence (sq_launch_lane_answers, called by sq_forward_impl
// with the block sq_resolve_pass resolved) and the stand-alone entry points (sqair_lane_*_test, sqair_lane_traj_score,
// sqair_lane_idf_solve, sqair_lane_hota_solve, sqair_lane_tracklog_smooth, sqair_lane_tracklog_score, sqair_lane_tracklog_fit, sqair_lane_tracklog_stitch).  Host code
// only: the kernels and their launchers live in sqair_lane.hip, which work here does not move.  A further follower is one member
// of SqLaneSet, its registration and builder here, and one line of sq_launch_lane_answers.
#include "sqair_internal.h"

// ------------------------------------------------------------------------------------------------
// what every user of one of the public structs checks, -1 + "<who>..." when a field is off
// ------------------------------------------------------------------------------------------------
static int sq_truth_slots_refusal(SqairHandle* h, const std::string& who, int G) {
  if (G >= 1 && G <= SQ_SCORE_MAXG) return 0;
  return sq_no(h, who + "G = " + std::to_string(G) + " must lie in 1.." + std::to_string(SQ_SCORE_MAXG));
}
static int sq_estimate_fields(SqairHandle* h, const std::string& who, const SqairLaneEstimate& e) {
  if (sq_unit_refusal(h, who, "iou_min", e.iou_min) != 0) return -1;
  if (!e.best_row) return sq_no(h, who + "best_row must not be NULL");
  return 0;
}
static int sq_layers_fields(SqairHandle* h, const std::string& who, const SqairLaneLayers& l) {
  if (sq_unit_refusal(h, who, "cover_min", l.cover_min) != 0) return -1;
  if (!l.match && !l.layer && !l.cover && !l.owner) return sq_no(h, who + "at least one of match, layer, cover and owner must be set");
  return 0;
}
static int sq_score_fields(SqairHandle* h, const std::string& who, const SqairLaneScore& c) {
  if (sq_truth_slots_refusal(h, who, c.G) != 0 || sq_unit_refusal(h, who, "iou_min", c.iou_min) != 0) return -1;
  if (!c.truth_box || !c.truth_present || !c.truth_valid || !c.counts || !c.iou_sum || !c.last_id)
    return sq_no(h, who + "truth_box, truth_present, truth_valid, counts, iou_sum and last_id must not be NULL");
  return 0;
}
static int sq_idf_fields(SqairHandle* h, const std::string& who, const SqairLaneIdf& c) {
  if (c.P < 1 || c.P > SQ_IDF_MAXP)
    return sq_no(h, who + "P = " + std::to_string(c.P) + " must lie in 1.." + std::to_string(SQ_IDF_MAXP));
  if (!c.col_id || !c.overlap || !c.row_frames || !c.col_frames || !c.extra_frames || !c.matched || !c.frag || !c.trk_state || !c.frames ||
      !c.totals)
    return sq_no(h, who + "col_id, overlap, row_frames, col_frames, extra_frames, matched, frag, trk_state, frames and totals must not be NULL");
  return 0;
}
static int sq_hota_fields(SqairHandle* h, const std::string& who, const SqairLaneHota& c) {
  if (c.P < 1 || c.P > SQ_HOTA_MAXP)
    return sq_no(h, who + "P = " + std::to_string(c.P) + " must lie in 1.." + std::to_string(SQ_HOTA_MAXP));
  if (c.L < 1 || c.L > SQ_HOTA_MAXL)
    return sq_no(h, who + "L = " + std::to_string(c.L) + " must lie in 1.." + std::to_string(SQ_HOTA_MAXL));
  if (!c.col_id || !c.log_q || !c.log_col || !c.log_row || !c.frames || !c.dropped_frames || !c.work || !c.totals_i || !c.totals_f ||
      !c.totals_c)
    return sq_no(h, who + "col_id, log_q, log_col, log_row, frames, dropped_frames, work, totals_i, totals_f and totals_c must not be NULL");
  return 0;
}
static int sq_identity_fields(SqairHandle* h, const std::string& who, const SqairLaneIdentity& c) {
  const int N = h->cfg.n_steps_per_image;
  if (c.M < N || c.M > SQ_IDENT_MAXM)
    return sq_no(h, who + "M = " + std::to_string(c.M) + " must lie in N = " + std::to_string(N) + ".." + std::to_string(SQ_IDENT_MAXM));
  if (sq_unit_refusal(h, who, "iou_min", c.iou_min) != 0) return -1;
  if (!(c.reid_dist >= 0.0f)) return sq_no(h, who + "reid_dist must be >= 0");                          // (NaN fails)
  if (!(c.reid_what > 0.0f)) return sq_no(h, who + "reid_what must lie in (0, +inf]");                  // (NaN fails)
  if (c.max_age < 0) return sq_no(h, who + "max_age must be >= 0");
  if (!c.trk_id || !c.trk_word || !c.trk_age || !c.trk_len || !c.trk_box || !c.next_id || !c.counts || !c.lane_id)
    return sq_no(h, who + "trk_id, trk_word, trk_age, trk_len, trk_box, next_id, counts and lane_id must not be NULL");
  return 0;
}
static int sq_tracklog_fields(SqairHandle* h, const std::string& who, const SqairLaneTrackLog& c) {
  if (c.L < 1 || c.L > SQ_TRACKLOG_MAXL)
    return sq_no(h, who + "L = " + std::to_string(c.L) + " must lie in 1.." + std::to_string(SQ_TRACKLOG_MAXL));
  if (!c.count || !c.log_valid || !c.log_id || !c.log_len || !c.log_box)
    return sq_no(h, who + "count, log_valid, log_id, log_len and log_box must not be NULL");
  return 0;
}
static int sq_motion_fields(SqairHandle* h, const std::string& who, const SqairLaneMotion& m) {
  const float v[4] = {m.q, m.r, m.v0_var, m.gate};
  const char* name[4] = {"q", "r", "v0_var", "gate"};
  for (int i = 0; i < 4; ++i)
    if (!(v[i] > 0.0f) || !std::isfinite(v[i])) return sq_no(h, who + name[i] + " must be finite and > 0");   // (NaN fails)
  if (!m.trk_kf || !m.velocity) return sq_no(h, who + "trk_kf and velocity must not be NULL");
  return 0;
}

// ------------------------------------------------------------------------------------------------
// registration: the handle's block, h->lane.  Switching the estimate off is h->lane = SqLaneSet{}: its followers go with it
// ------------------------------------------------------------------------------------------------
static void sq_layers_off(SqLaneSet& l) { l.lay_on = false; l.lay = SqairLaneLayers{}; }
// (the score reads the identity's ids only while both are on: either going off puts score_ids back to 0)
// (and the IDF reads the score's truth and its truth_match: it goes off with it)
static void sq_idf_off(SqLaneSet& l) { l.idf_on = false; l.idf = SqairLaneIdf{}; }
// (and so does the HOTA log: the truth and the id words are the score's)
static void sq_hota_off(SqLaneSet& l) { l.hota_on = false; l.hota = SqairLaneHota{}; }
static void sq_score_off(SqLaneSet& l) { l.score_on = false; l.score = SqairLaneScore{}; l.score_ids = false; sq_idf_off(l); sq_hota_off(l); }
// (the motion filter is a mode of the identity's launch: it goes off with it)
static void sq_motion_off(SqLaneSet& l) { l.motion_on = false; l.motion = SqairLaneMotion{}; }
// (and so does the track log: the ids and lengths it copies are the identity's)
static void sq_tracklog_off(SqLaneSet& l) { l.tracklog_on = false; l.tracklog = SqairLaneTrackLog{}; }
static void sq_identity_off(SqLaneSet& l) {
  l.ident_on = false; l.ident = SqairLaneIdentity{}; l.score_ids = false;
  sq_motion_off(l); sq_tracklog_off(l);
}
// what the followers need of the estimate they read (best_row is never NULL in a registered estimate; `what`: the identity keeps an
// appearance, trk_what, and reads the estimate's)
static bool sq_estimate_scorable(const SqairLaneEstimate& e) { return e.box && e.presence && e.obj_id && e.map_count; }
static bool sq_estimate_identifiable(const SqairLaneEstimate& e, bool what) {
  return e.box && e.presence && e.obj_id && e.best_row && (!what || e.what);
}
static int sq_estimate_smc_mismatch(SqairHandle* h, const std::string& who, const SqairLaneEstimate& e) {
  if (!h->smc_on || e.log_w == h->smc.log_w) return 0;
  return sq_no(h, who + "with SMC on (sqair_set_smc) log_w must be smc->log_w, the carried log weights of the pass's rows");
}
// what every follower's registration checks after its own needs of the estimate: the estimate's T, the state's B
static int sq_follower_shape_refusal(SqairHandle* h, const std::string& who, int T, int B) {
  if (T != h->lane.est_T)
    return sq_no(h, who + "T = " + std::to_string(T) + " but the estimate set by sqair_set_estimate is for T = " + std::to_string(h->lane.est_T));
  return sq_state_b_mismatch(h, who, B);
}
extern "C" int sqair_set_estimate(SqairHandle* h, const SqairLaneEstimate* est, int T, int B) {
  if (!h) return -1;
  if (!est) {
    h->lane = SqLaneSet{};
    return 0;
  }
  const std::string who = "sqair_set_estimate: ";
  if (!h->state_on) return sq_no(h, who + "needs a carried state (sqair_set_state): the estimate weighs the rows it carries");
  if (T < 1) return sq_no(h, who + "T must be >= 1");
  if (sq_state_b_mismatch(h, who, B) != 0) return -1;
  if (sq_estimate_fields(h, who, *est) != 0 || sq_estimate_smc_mismatch(h, who, *est) != 0) return -1;
  // a re-registered estimate drops the followers it can no longer feed: outputs sized for the other T, outputs they read gone
  SqLaneSet& l = h->lane;
  if (T != l.est_T) sq_layers_off(l);
  if (T != l.est_T || !sq_estimate_scorable(*est)) sq_score_off(l);
  if (T != l.est_T || !sq_estimate_identifiable(*est, l.ident.trk_what != nullptr)) sq_identity_off(l);
  l.est_on = true; l.est = *est; l.est_T = T;
  return 0;
}
int sq_estimate_refusal(SqairHandle* h, int T, const SqairOutputs* outp) {
  if (!h->state_on || !h->lane.est_on) return 0;
  const std::string who = "lane estimate (sqair_set_estimate): ";
  if (T != h->lane.est_T)
    return sq_no(h, who + "the outputs were registered for passes of T = " + std::to_string(h->lane.est_T) + " frames, a pass of T = " +
                    std::to_string(T) + " cannot fill them");
  if (!outp || !outp->log_weights_per_timestep)
    return sq_no(h, who + "the weights are formed from log_weights_per_timestep: a pass with the estimate on must bind that output");
  if (h->lane.est.mean_canvas && !outp->canvas) return sq_no(h, who + "mean_canvas averages the pass's canvases: the pass must bind out->canvas");
  return sq_estimate_smc_mismatch(h, who, h->lane.est);
}
extern "C" int sqair_set_layers(SqairHandle* h, const SqairLaneLayers* lay, int T, int B) {
  if (!h) return -1;
  if (!lay) {
    sq_layers_off(h->lane);
    return 0;
  }
  const std::string who = "sqair_set_layers: ";
  if (!h->state_on || !h->lane.est_on)
    return sq_no(h, who + "needs an estimate (sqair_set_estimate): the layers weigh and associate the particles as it does");
  if (sq_follower_shape_refusal(h, who, T, B) != 0 || sq_layers_fields(h, who, *lay) != 0) return -1;
  h->lane.lay_on = true; h->lane.lay = *lay;
  return 0;
}
extern "C" int sqair_set_score(SqairHandle* h, const SqairLaneScore* score, int T, int B) {
  if (!h) return -1;
  if (!score) {
    sq_score_off(h->lane);
    return 0;
  }
  const std::string who = "sqair_set_score: ";
  if (!h->state_on || !h->lane.est_on)
    return sq_no(h, who + "needs an estimate (sqair_set_estimate): the score reads the lane answer it writes");
  if (!sq_estimate_scorable(h->lane.est))
    return sq_no(h, who + "the estimate (sqair_set_estimate) must bind box, presence, obj_id and map_count: the score reads them");
  if (sq_follower_shape_refusal(h, who, T, B) != 0 || sq_score_fields(h, who, *score) != 0) return -1;
  // a re-registered score drops the IDF it can no longer feed: a table sized for the other G, the output it reads gone
  if (h->lane.score_on && (!score->truth_match || score->G != h->lane.score.G)) sq_idf_off(h->lane);
  if (h->lane.score_on && score->G != h->lane.score.G) sq_hota_off(h->lane);   // (a log sized for the other G)
  h->lane.score_on = true; h->lane.score = *score;
  return 0;
}
extern "C" int sqair_set_idf(SqairHandle* h, const SqairLaneIdf* idf, int T, int B) {
  if (!h) return -1;
  if (!idf) {
    sq_idf_off(h->lane);
    return 0;
  }
  const std::string who = "sqair_set_idf: ";
  if (!h->state_on || !h->lane.est_on || !h->lane.score_on)
    return sq_no(h, who + "needs a score (sqair_set_score): the table is keyed by the truth and the id words the score reads");
  if (!h->lane.score.truth_match)
    return sq_no(h, who + "the score (sqair_set_score) must bind truth_match: the trajectory statistics read the score's matches");
  if (sq_follower_shape_refusal(h, who, T, B) != 0 || sq_idf_fields(h, who, *idf) != 0) return -1;
  h->lane.idf_on = true; h->lane.idf = *idf;
  return 0;
}
extern "C" int sqair_set_hota(SqairHandle* h, const SqairLaneHota* hota, int T, int B) {
  if (!h) return -1;
  if (!hota) {
    sq_hota_off(h->lane);
    return 0;
  }
  const std::string who = "sqair_set_hota: ";
  if (!h->state_on || !h->lane.est_on || !h->lane.score_on)
    return sq_no(h, who + "needs a score (sqair_set_score): the log is keyed by the truth and the id words the score reads");
  if (sq_follower_shape_refusal(h, who, T, B) != 0 || sq_hota_fields(h, who, *hota) != 0) return -1;
  h->lane.hota_on = true; h->lane.hota = *hota;
  return 0;
}
extern "C" int sqair_set_identity(SqairHandle* h, const SqairLaneIdentity* id, int T, int B) {
  if (!h) return -1;
  if (!id) {
    sq_identity_off(h->lane);
    return 0;
  }
  const std::string who = "sqair_set_identity: ";
  if (!h->state_on || !h->lane.est_on)
    return sq_no(h, who + "needs an estimate (sqair_set_estimate): the identity links the lane answer it writes");
  if (!sq_estimate_identifiable(h->lane.est, false))
    return sq_no(h, who + "the estimate (sqair_set_estimate) must bind box, presence, obj_id and best_row: the identity reads them");
  if (id->trk_what && !h->lane.est.what)
    return sq_no(h, who + "trk_what needs the estimate (sqair_set_estimate) to bind what: the appearance it remembers");
  if (sq_follower_shape_refusal(h, who, T, B) != 0 || sq_identity_fields(h, who, *id) != 0) return -1;
  if (!id->track_len) sq_tracklog_off(h->lane);   // (a re-registered identity drops the log it can no longer feed)
  h->lane.ident_on = true; h->lane.ident = *id;
  return 0;
}
extern "C" int sqair_set_tracklog(SqairHandle* h, const SqairLaneTrackLog* log, int T, int B) {
  if (!h) return -1;
  if (!log) {
    sq_tracklog_off(h->lane);
    return 0;
  }
  const std::string who = "sqair_set_tracklog: ";
  if (!h->state_on || !h->lane.est_on || !h->lane.ident_on)
    return sq_no(h, who + "needs an identity (sqair_set_identity): the log is keyed by the lane_id it writes");
  if (!h->lane.ident.track_len)
    return sq_no(h, who + "the identity (sqair_set_identity) must bind track_len: the log records it");
  if (sq_follower_shape_refusal(h, who, T, B) != 0 || sq_tracklog_fields(h, who, *log) != 0) return -1;
  h->lane.tracklog_on = true; h->lane.tracklog = *log;
  return 0;
}
extern "C" int sqair_set_motion(SqairHandle* h, const SqairLaneMotion* m, int T, int B) {
  if (!h) return -1;
  if (!m) {
    sq_motion_off(h->lane);
    return 0;
  }
  const std::string who = "sqair_set_motion: ";
  if (!h->state_on || !h->lane.est_on || !h->lane.ident_on)
    return sq_no(h, who + "needs an identity (sqair_set_identity): the filter lives in the track table it keeps");
  if (sq_follower_shape_refusal(h, who, T, B) != 0 || sq_motion_fields(h, who, *m) != 0) return -1;
  h->lane.motion_on = true; h->lane.motion = *m;
  return 0;
}
// per-frame matching (include/sqair_hip.h: sqair_set_lane_match): a plain setting of the handle, no registration; the pass reads it
// through its resolved block (sq_resolve_pass), the stand-alone entry points read it at their launch
extern "C" int sqair_set_lane_match(SqairHandle* h, int score, int identity, int traj_link) {
  if (!h) return -1;
  const int v[3] = {score, identity, traj_link};
  const char* name[3] = {"score", "identity", "traj_link"};
  for (int i = 0; i < 3; ++i)
    if (v[i] != 0 && v[i] != 1)
      return sq_no(h, std::string("sqair_set_lane_match: ") + name[i] + " = " + std::to_string(v[i]) +
                          " must be 0 (keep + greedy) or 1 (keep + optimal)");
  h->match_score = score; h->match_ident = identity; h->match_traj = traj_link;
  return 0;
}
extern "C" int sqair_set_score_ids(SqairHandle* h, int lane_ids) {
  if (!h) return -1;
  if (lane_ids && !(h->state_on && h->lane.est_on && h->lane.score_on && h->lane.ident_on))
    return sq_no(h, "sqair_set_score_ids: needs both a score (sqair_set_score) and an identity (sqair_set_identity): the score reads "
                    "the lane_id the identity writes");
  h->lane.score_ids = lane_ids != 0;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// the kernels' arguments, one builder each: the pass (sq_launch_lane_answers) and the kernel-level entry points both call these
// ------------------------------------------------------------------------------------------------
static LaneEstArgs sq_estimate_args(const SqairConfig& c, const LaneRows& rows, const float* what, int what_ld, const float* canvas,
                                    const float* lw, const SqairLaneEstimate& est, int T, int B, int K) {
  LaneEstArgs a; memset(&a, 0, sizeof(a));
  a.rows = rows;
  a.what = what; a.what_ld = what_ld; a.canvas = canvas; a.lw = lw; a.est = est;
  a.T = T; a.B = B; a.K = K; a.N = c.n_steps_per_image; a.nw = c.n_what; a.H = c.img_h; a.W = c.img_w;
  return a;
}
static LaneLayerArgs sq_layers_args(const SqairConfig& c, const LaneRows& rows, const float* glimpse, const float* lw, const float* log_w,
                                    float iou_min, const SqairLaneLayers& lay, int T, int B, int K) {
  LaneLayerArgs a; memset(&a, 0, sizeof(a));
  a.rows = rows;
  a.glimpse = glimpse; a.lw = lw; a.log_w = log_w; a.iou_min = iou_min; a.lay = lay;
  a.T = T; a.B = B; a.K = K; a.N = c.n_steps_per_image; a.G = c.glimpse_size; a.H = c.img_h; a.W = c.img_w;
  return a;
}
// (`what` is read only by an identity that keeps an appearance, trk_what)
static LaneIdentArgs sq_identity_args(const SqairConfig& c, const float* box, const float* presence, const float* obj_id, const float* what,
                                      const int32_t* best_row, const SqairLaneIdentity& id, int T, int B, int match,
                                      const SqairLaneMotion* motion = nullptr) {
  LaneIdentArgs a; memset(&a, 0, sizeof(a));
  a.box = box; a.presence = presence; a.obj_id = obj_id; a.best_row = best_row; a.what = id.trk_what ? what : nullptr; a.id = id;
  a.T = T; a.B = B; a.N = c.n_steps_per_image; a.nw = c.n_what; a.match = match;
  if (motion) { a.motion = 1; a.mo = *motion; }
  return a;
}
static LaneScoreArgs sq_score_args(const SqairConfig& c, const float* box, const float* presence, const float* obj_id,
                                   const int32_t* map_count, const SqairLaneScore& score, int T, int B, int match) {
  LaneScoreArgs a; memset(&a, 0, sizeof(a));
  a.box = box; a.presence = presence; a.obj_id = obj_id; a.map_count = map_count; a.sc = score;
  a.T = T; a.B = B; a.N = c.n_steps_per_image; a.match = match;
  return a;
}
// (`ids`: the id words the score is handed for the same frames; of `score` the truth, iou_min, G and truth_match are read)
static LaneIdfArgs sq_idf_args(const SqairConfig& c, const float* box, const float* presence, const float* ids, const int32_t* map_count,
                               const SqairLaneScore& score, const SqairLaneIdf& idf, int T, int B) {
  LaneIdfArgs a; memset(&a, 0, sizeof(a));
  a.box = box; a.presence = presence; a.ids = ids; a.map_count = map_count; a.sc = score; a.idf = idf;
  a.T = T; a.B = B; a.N = c.n_steps_per_image;
  return a;
}
// (`ids`: as for the IDF; of `score` the truth and G are read)
static LaneHotaArgs sq_hota_args(const SqairConfig& c, const float* box, const float* presence, const float* ids, const int32_t* map_count,
                                 const SqairLaneScore& score, const SqairLaneHota& hota, int T, int B) {
  LaneHotaArgs a; memset(&a, 0, sizeof(a));
  a.box = box; a.presence = presence; a.ids = ids; a.map_count = map_count; a.sc = score; a.hota = hota;
  a.T = T; a.B = B; a.N = c.n_steps_per_image;
  return a;
}

static LaneTrackLogArgs sq_tracklog_args(const SqairConfig& c, const int32_t* lane_id, const int32_t* track_len, const int32_t* best_row,
                                         const float* box, const SqairLaneTrackLog& log, int T, int B) {
  LaneTrackLogArgs a; memset(&a, 0, sizeof(a));
  a.lane_id = lane_id; a.track_len = track_len; a.best_row = best_row; a.box = box; a.log = log;
  a.T = T; a.B = B; a.N = c.n_steps_per_image;
  return a;
}

// ------------------------------------------------------------------------------------------------
// the pass: every lane launch, in the one order they have.  The estimate comes before the resampler zeroes the weights it reads
// and rewrites the map; the followers read the estimate's own output buffers, the identity before the score, which may read the
// ids it writes, the IDF1 table after the score, whose matches and id words it reads.  `l` is the pass's resolved copy: nothing here reads the handle's registration
// ------------------------------------------------------------------------------------------------
int sq_launch_lane_answers(SqairHandle* h, const SqLaneSet& l, const float* rec, const float* glimpse, const SqairOutputs& out, int T, int B,
                           hipStream_t s) {
  if (!l.est_on) return 0;   // (no follower without it)
  const SqairConfig& c = h->cfg;
  const int K = c.k_particles;
  const SqairLaneEstimate& e = l.est;
  const float* lw = out.log_weights_per_timestep;
  // lane estimates: one answer per (frame, lane) from this pass's rows and the log weights they carry (sqair_set_estimate)
  sq_launch_lane_estimate(sq_estimate_args(c, LaneRows{rec + rec::WHERE, rec::W, rec + rec::PRES, rec::W, rec + rec::ID, rec::W, 1},
                                           rec + rec::WHAT, rec::W, out.canvas, lw, e, T, B, K), s);
  // object layers: the decoder's sum over slots taken apart per object of the lane (sqair_set_layers), by the estimate's weights
  // and association
  if (l.lay_on &&
      sq_launch_lane_layers(sq_layers_args(c, LaneRows{rec + rec::WHERE, rec::W, rec + rec::PRES, rec::W, nullptr, 0, 1}, glimpse, lw,
                                           e.log_w, e.iou_min, l.lay, T, B, K), s) != 0) {
    sq_set_error(h, "sqair_forward: the object layers launch failed (dynamic LDS limit)");
    return -2;
  }
  // lane identities: the lane's objects linked to the lane's track table (sqair_set_identity), updated in place
  // (sqair_set_motion: the same node, in its motion instantiation)
  if (l.ident_on)
    sq_launch_lane_identity(sq_identity_args(c, e.box, e.presence, e.obj_id, e.what, e.best_row, l.ident, T, B, l.ident_match,
                                             l.motion_on ? &l.motion : nullptr), s);
  // the track log: the frame's lane_id, track_len and box words into the lane's ring (sqair_set_tracklog), right behind their writer
  if (l.ident_on && l.tracklog_on)
    sq_launch_lane_tracklog(sq_tracklog_args(c, l.ident.lane_id, l.ident.track_len, e.best_row, e.box, l.tracklog, T, B), s);
  // stream scoring: the lane answer against the caller's ground truth (sqair_set_score), accumulated in place.  sqair_set_score_ids:
  // the kernel takes the id as a 32-bit word, so the identity's int32 lane_id stands where obj_id stands
  if (l.score_on) {
    const float* ids = (l.ident_on && l.score_ids) ? reinterpret_cast<const float*>(l.ident.lane_id) : e.obj_id;
    sq_launch_lane_score(sq_score_args(c, e.box, e.presence, ids, e.map_count, l.score, T, B, l.score_match), s);
    // IDF1 scoring: the clip's identity overlap table (sqair_set_idf), accumulated in place on the words the score just read
    if (l.idf_on) sq_launch_lane_idf(sq_idf_args(c, e.box, e.presence, ids, e.map_count, l.score, l.idf, T, B), s);
    // HOTA scoring: one record of the clip log per scored frame (sqair_set_hota), on the same words
    if (l.hota_on) sq_launch_lane_hota(sq_hota_args(c, e.box, e.presence, ids, e.map_count, l.score, l.hota, T, B), s);
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// kernel-level checks (tests/test_{estimate,layers,score,identity,idf}_kernel.py): one kernel on caller tensors, no state and no pass;
// K, where there is one, is given (1..SQ_MAX_K)
// ------------------------------------------------------------------------------------------------
extern "C" int sqair_lane_estimate_test(SqairHandle* h, const float* where, const float* presence, const float* obj_id,
                                        const float* what, const float* canvas, const float* lw, int T, int B, int K,
                                        const SqairLaneEstimate* est, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_estimate_test: ";
  if (!where || !presence || !obj_id || !lw || !est || T < 1 || B < 1 || K < 1 || K > SQ_MAX_K || T > 65535 ||
      (int64_t)B * K > INT32_MAX)
    return sq_no(h, who + "null where / presence / obj_id / lw / est or bad T / B / K (1 <= K <= " + std::to_string(SQ_MAX_K) + ")");
  if (sq_estimate_fields(h, who, *est) != 0) return -1;
  if (est->what && !what) return sq_no(h, who + "est->what needs what");
  if (est->mean_canvas && !canvas) return sq_no(h, who + "est->mean_canvas needs canvas");
  sq_launch_lane_estimate(sq_estimate_args(h->cfg, LaneRows{where, 4, presence, 1, obj_id, 1, 1}, what, h->cfg.n_what, canvas, lw, *est,
                                           T, B, K), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int sqair_lane_layers_test(SqairHandle* h, const float* glimpse, const float* where, const float* presence, const float* lw,
                                      const float* log_w, float iou_min, int T, int B, int K, const SqairLaneLayers* lay, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_layers_test: ";
  if (!glimpse || !where || !presence || !lw || !lay || T < 1 || B < 1 || K < 1 || K > SQ_MAX_K || T > 65535 || (int64_t)B * K > INT32_MAX)
    return sq_no(h, who + "null glimpse / where / presence / lw / lay or bad T / B / K (1 <= K <= " + std::to_string(SQ_MAX_K) + ")");
  if (sq_unit_refusal(h, who, "iou_min", iou_min) != 0 || sq_layers_fields(h, who, *lay) != 0) return -1;
  if (sq_launch_lane_layers(sq_layers_args(h->cfg, LaneRows{where, 4, presence, 1, nullptr, 0, 1}, glimpse, lw, log_w, iou_min, *lay,
                                           T, B, K), (hipStream_t)stream) != 0) {
    sq_set_error(h, who + "the launch failed (dynamic LDS limit)");
    return -2;
  }
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int sqair_lane_score_test(SqairHandle* h, const float* box, const float* presence, const float* obj_id, const int32_t* map_count,
                                     int T, int B, const SqairLaneScore* score, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_score_test: ";
  if (!box || !presence || !obj_id || !map_count || !score || T < 1 || B < 1 || T > 65535)
    return sq_no(h, who + "null box / presence / obj_id / map_count / score or bad T / B");
  if (sq_score_fields(h, who, *score) != 0) return -1;
  sq_launch_lane_score(sq_score_args(h->cfg, box, presence, obj_id, map_count, *score, T, B, h->match_score), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int sqair_lane_identity_test(SqairHandle* h, const float* box, const float* presence, const float* obj_id, const float* what,
                                        const int32_t* best_row, int T, int B, const SqairLaneIdentity* id, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_identity_test: ";
  if (!box || !presence || !obj_id || !best_row || !id || T < 1 || B < 1 || T > 65535)
    return sq_no(h, who + "null box / presence / obj_id / best_row / id or bad T / B");
  if (sq_identity_fields(h, who, *id) != 0) return -1;
  if (id->trk_what && !what) return sq_no(h, who + "id->trk_what needs what");
  sq_launch_lane_identity(sq_identity_args(h->cfg, box, presence, obj_id, what, best_row, *id, T, B, h->match_ident), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int sqair_lane_identity_motion_test(SqairHandle* h, const float* box, const float* presence, const float* obj_id, const float* what,
                                               const int32_t* best_row, int T, int B, const SqairLaneIdentity* id, const SqairLaneMotion* m,
                                               void* stream) {
  if (!h) return -1;
  if (!m) return sqair_lane_identity_test(h, box, presence, obj_id, what, best_row, T, B, id, stream);
  const std::string who = "sqair_lane_identity_motion_test: ";
  if (!box || !presence || !obj_id || !best_row || !id || T < 1 || B < 1 || T > 65535)
    return sq_no(h, who + "null box / presence / obj_id / best_row / id or bad T / B");
  if (sq_identity_fields(h, who, *id) != 0 || sq_motion_fields(h, who, *m) != 0) return -1;
  if (id->trk_what && !what) return sq_no(h, who + "id->trk_what needs what");
  sq_launch_lane_identity(sq_identity_args(h->cfg, box, presence, obj_id, what, best_row, *id, T, B, h->match_ident, m), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int sqair_lane_idf_test(SqairHandle* h, const float* box, const float* presence, const float* ids, const int32_t* map_count,
                                   int T, int B, const SqairLaneScore* score, const SqairLaneIdf* idf, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_idf_test: ";
  if (!box || !presence || !ids || !map_count || !score || !idf || T < 1 || B < 1 || T > 65535)
    return sq_no(h, who + "null box / presence / ids / map_count / score / idf or bad T / B");
  if (sq_truth_slots_refusal(h, who, score->G) != 0 || sq_unit_refusal(h, who, "iou_min", score->iou_min) != 0) return -1;
  if (!score->truth_box || !score->truth_present || !score->truth_valid || !score->truth_match)
    return sq_no(h, who + "the score's truth_box, truth_present, truth_valid and truth_match must not be NULL");
  if (sq_idf_fields(h, who, *idf) != 0) return -1;
  sq_launch_lane_idf(sq_idf_args(h->cfg, box, presence, ids, map_count, *score, *idf, T, B), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// the IDF1 solve (include/sqair_hip.h: sqair_lane_idf_solve): a stand-alone call on the table the passes -- or a test -- filled, nothing
// registered on the handle, which gives the error text
extern "C" int sqair_lane_idf_solve(SqairHandle* h, const SqairLaneIdf* idf, int G, int B, const int32_t* close, int64_t* open,
                                    int32_t* assign, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_idf_solve: ";
  if (!idf) return sq_no(h, who + "idf must not be NULL");
  if (B < 1) return sq_no(h, who + "B = " + std::to_string(B) + " must be >= 1");
  if (sq_truth_slots_refusal(h, who, G) != 0 || sq_idf_fields(h, who, *idf) != 0) return -1;
  LaneIdfSolveArgs a; memset(&a, 0, sizeof(a));
  a.idf = *idf; a.close = close; a.open = open; a.assign = assign; a.G = G; a.B = B;
  sq_launch_lane_idf_solve(a, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int sqair_lane_hota_test(SqairHandle* h, const float* box, const float* presence, const float* ids, const int32_t* map_count,
                                    int T, int B, const SqairLaneScore* score, const SqairLaneHota* hota, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_hota_test: ";
  if (!box || !presence || !ids || !map_count || !score || !hota || T < 1 || B < 1 || T > 65535)
    return sq_no(h, who + "null box / presence / ids / map_count / score / hota or bad T / B");
  if (sq_truth_slots_refusal(h, who, score->G) != 0) return -1;
  if (!score->truth_box || !score->truth_present || !score->truth_valid)
    return sq_no(h, who + "the score's truth_box, truth_present and truth_valid must not be NULL");
  if (sq_hota_fields(h, who, *hota) != 0) return -1;
  sq_launch_lane_hota(sq_hota_args(h->cfg, box, presence, ids, map_count, *score, *hota, T, B), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// the HOTA solve (include/sqair_hip.h: sqair_lane_hota_solve): a stand-alone call on the log the passes -- or a test -- filled, nothing
// registered on the handle, which gives the error text
extern "C" int sqair_lane_hota_solve(SqairHandle* h, const SqairLaneHota* hota, int G, int N, int B, const int32_t* close, int64_t* open_i,
                                     double* open_f, int64_t* open_c, int32_t* match, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_hota_solve: ";
  if (!hota) return sq_no(h, who + "hota must not be NULL");
  if (B < 1) return sq_no(h, who + "B = " + std::to_string(B) + " must be >= 1");
  if (N < 1 || N > 16) return sq_no(h, who + "N = " + std::to_string(N) + " must lie in 1..16");
  if (sq_truth_slots_refusal(h, who, G) != 0 || sq_hota_fields(h, who, *hota) != 0) return -1;
  LaneHotaSolveArgs a; memset(&a, 0, sizeof(a));
  a.hota = *hota; a.close = close; a.open_i = open_i; a.open_f = open_f; a.open_c = open_c; a.match = match; a.G = G; a.N = N; a.B = B;
  sq_launch_lane_hota_solve(a, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
extern "C" int sqair_lane_tracklog_test(SqairHandle* h, const int32_t* lane_id, const int32_t* track_len, const int32_t* best_row,
                                        const float* box, int T, int B, const SqairLaneTrackLog* log, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_tracklog_test: ";
  if (!lane_id || !track_len || !best_row || !box || !log || T < 1 || B < 1 || T > 65535)
    return sq_no(h, who + "null lane_id / track_len / best_row / box / log or bad T / B");
  if (sq_tracklog_fields(h, who, *log) != 0) return -1;
  sq_launch_lane_tracklog(sq_tracklog_args(h->cfg, lane_id, track_len, best_row, box, *log, T, B), (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// the track log's solve (include/sqair_hip.h: sqair_lane_tracklog_smooth): a stand-alone call on the log the passes -- or a test --
// filled, nothing registered on the handle, which gives the error text.  ONE statement of what it accepts, the scratch query's too
static const char* sq_tracklog_shape_refusal(int lag, int C, int N) {
  if (lag < 1 || lag > SQ_TRACKLOG_MAXL) return "lag must lie in 1..L";
  if (C < 1 || C > SQ_TRACKLOG_MAXC) return "C must lie in 1..64";
  if (N < 1 || N > 16) return "N must lie in 1..16";
  return nullptr;
}
extern "C" int64_t sqair_lane_tracklog_work_bytes(int lag, int C, int N) {
  if (sq_tracklog_shape_refusal(lag, C, N)) return 0;
  return (int64_t)lag * C * (int64_t)sizeof(int32_t);
}
extern "C" int sqair_lane_tracklog_smooth(SqairHandle* h, const SqairLaneTrackLog* log, int lag, int C, int N, int B, float q, float r,
                                          float v0_var, const SqairTrackLogOut* out, void* work, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_tracklog_smooth: ";
  if (!log || !out || !work) return sq_no(h, who + "log, out and work must not be NULL");
  if (B < 1) return sq_no(h, who + "B = " + std::to_string(B) + " must be >= 1");
  if (sq_tracklog_fields(h, who, *log) != 0) return -1;
  if (const char* why = sq_tracklog_shape_refusal(lag, C, N))
    return sq_no(h, who + why + " (lag = " + std::to_string(lag) + ", L = " + std::to_string(log->L) + ", C = " + std::to_string(C) +
                        ", N = " + std::to_string(N) + ")");
  if (lag > log->L) return sq_no(h, who + "lag = " + std::to_string(lag) + " must lie in 1..L = " + std::to_string(log->L));
  const float v[3] = {q, r, v0_var};
  const char* name[3] = {"q", "r", "v0_var"};
  for (int i = 0; i < 3; ++i)
    if (!(v[i] > 0.0f) || !std::isfinite(v[i])) return sq_no(h, who + name[i] + " must be finite and > 0");   // (NaN fails)
  if (!out->track_id || !out->n_tracks || !out->len0 || !out->frame_index || !out->state || !out->size || !out->filt || !out->smooth)
    return sq_no(h, who + "track_id, n_tracks, len0, frame_index, state, size, filt and smooth must not be NULL");
  LaneTrackLogSmoothArgs a; memset(&a, 0, sizeof(a));
  a.log = *log; a.out = *out; a.work = (int32_t*)work; a.q = q; a.r = r; a.v0_var = v0_var; a.lag = lag; a.C = C; a.N = N; a.B = B;
  sq_launch_lane_tracklog_smooth(a, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// track log scoring (include/sqair_hip.h: sqair_lane_tracklog_score): a stand-alone call on the table the solve wrote -- or on a test's
// tensors --, nothing registered on the handle, which gives the error text
extern "C" int sqair_lane_tracklog_score(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table,
                                         const SqairTrackLogTruth* truth, const SqairTrackLogScore* score, int lag, int C, int B, int match,
                                         void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_tracklog_score: ";
  if (!log || !table || !truth || !score) return sq_no(h, who + "log, table, truth and score must not be NULL");
  if (B < 1) return sq_no(h, who + "B = " + std::to_string(B) + " must be >= 1");
  if (sq_tracklog_fields(h, who, *log) != 0) return -1;
  if (lag < 1 || lag > log->L) return sq_no(h, who + "lag = " + std::to_string(lag) + " must lie in 1..L = " + std::to_string(log->L));
  if (C < 1 || C > SQ_TRACKLOG_MAXC) return sq_no(h, who + "C = " + std::to_string(C) + " must lie in 1..64");
  if (sq_truth_slots_refusal(h, who, truth->G) != 0 || sq_unit_refusal(h, who, "iou_min", score->iou_min) != 0) return -1;
  if (match != 0 && match != 1) return sq_no(h, who + "match = " + std::to_string(match) + " must be 0 (greedy) or 1 (optimal)");
  if (!table->track_id || !table->frame_index || !table->state || !table->size || !table->filt || !table->smooth)
    return sq_no(h, who + "the table's track_id, frame_index, state, size, filt and smooth must not be NULL");
  if (!truth->truth_box || !truth->truth_present || !truth->truth_valid)
    return sq_no(h, who + "truth_box, truth_present and truth_valid must not be NULL");
  if (!score->counts || !score->sums) return sq_no(h, who + "counts and sums must not be NULL");
  LaneTrackLogScoreArgs a; memset(&a, 0, sizeof(a));
  a.log = *log; a.tab = *table; a.tr = *truth; a.sc = *score; a.lag = lag; a.C = C; a.B = B; a.match = match;
  sq_launch_lane_tracklog_score(a, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// motion calibration (include/sqair_hip.h: sqair_lane_tracklog_fit): a stand-alone call on the table and the slots the solve wrote --
// or on a test's tensors --, nothing registered on the handle, which gives the error text
extern "C" int sqair_lane_tracklog_fit(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table, const void* work,
                                       const SqairTrackLogFit* fit, int lag, int C, int N, int B, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_tracklog_fit: ";
  if (!log || !table || !work || !fit) return sq_no(h, who + "log, table, work and fit must not be NULL");
  if (B < 1) return sq_no(h, who + "B = " + std::to_string(B) + " must be >= 1");
  if (sq_tracklog_fields(h, who, *log) != 0) return -1;
  if (const char* why = sq_tracklog_shape_refusal(lag, C, N))
    return sq_no(h, who + why + " (lag = " + std::to_string(lag) + ", L = " + std::to_string(log->L) + ", C = " + std::to_string(C) +
                        ", N = " + std::to_string(N) + ")");
  if (lag > log->L) return sq_no(h, who + "lag = " + std::to_string(lag) + " must lie in 1..L = " + std::to_string(log->L));
  if (fit->Q < 1 || fit->Q > SQAIR_TRACKLOG_FIT_MAX_GRID || fit->R < 1 || fit->R > SQAIR_TRACKLOG_FIT_MAX_GRID)
    return sq_no(h, who + "Q = " + std::to_string(fit->Q) + " and R = " + std::to_string(fit->R) + " must lie in 1..16");
  if (fit->burn < 0) return sq_no(h, who + "burn = " + std::to_string(fit->burn) + " must be >= 0");
  auto positive = [](float v) { return v > 0.0f && std::isfinite(v); };   // (NaN fails)
  if (!positive(fit->v0_var)) return sq_no(h, who + "v0_var must be finite and > 0");
  for (int i = 0; i < fit->Q; ++i)
    if (!positive(fit->q[i])) return sq_no(h, who + "q[" + std::to_string(i) + "] must be finite and > 0");
  for (int i = 0; i < fit->R; ++i)
    if (!positive(fit->r[i])) return sq_no(h, who + "r[" + std::to_string(i) + "] must be finite and > 0");
  if (!table->frame_index || !table->state) return sq_no(h, who + "the table's frame_index and state must not be NULL");
  if (!fit->counts || !fit->sums) return sq_no(h, who + "counts and sums must not be NULL");
  LaneTrackLogFitArgs a; memset(&a, 0, sizeof(a));
  a.log = *log; a.tab = *table; a.work = (const int32_t*)work; a.fit = *fit; a.lag = lag; a.C = C; a.N = N; a.B = B;
  sq_launch_lane_tracklog_fit(a, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// track log stitching (include/sqair_hip.h: sqair_lane_tracklog_stitch): a stand-alone call on the table and the slots the solve wrote
// -- or on a test's tensors --, nothing registered on the handle, which gives the error text
extern "C" int sqair_lane_tracklog_stitch(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table, const void* work,
                                          int lag, int C, int N, int B, float q, float r, float v0_var, const SqairTrackLogStitch* stitch,
                                          const SqairTrackLogOut* stitched, void* work_out, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_tracklog_stitch: ";
  if (!log || !table || !work || !stitch || !stitched || !work_out)
    return sq_no(h, who + "log, table, work, stitch, stitched and work_out must not be NULL");
  if (B < 1) return sq_no(h, who + "B = " + std::to_string(B) + " must be >= 1");
  if (sq_tracklog_fields(h, who, *log) != 0) return -1;
  if (const char* why = sq_tracklog_shape_refusal(lag, C, N))
    return sq_no(h, who + why + " (lag = " + std::to_string(lag) + ", L = " + std::to_string(log->L) + ", C = " + std::to_string(C) +
                        ", N = " + std::to_string(N) + ")");
  if (lag > log->L) return sq_no(h, who + "lag = " + std::to_string(lag) + " must lie in 1..L = " + std::to_string(log->L));
  const float v[4] = {q, r, v0_var, stitch->gate};
  const char* name[4] = {"q", "r", "v0_var", "gate"};
  for (int i = 0; i < 4; ++i)
    if (!(v[i] > 0.0f) || !std::isfinite(v[i])) return sq_no(h, who + name[i] + " must be finite and > 0");   // (NaN fails)
  if (stitch->max_gap < 0 || stitch->max_gap > lag)
    return sq_no(h, who + "max_gap = " + std::to_string(stitch->max_gap) + " must lie in 0..lag = " + std::to_string(lag));
  if (!table->track_id || !table->n_tracks || !table->len0 || !table->frame_index || !table->state || !table->filt || !table->smooth)
    return sq_no(h, who + "the table's track_id, n_tracks, len0, frame_index, state, filt and smooth must not be NULL");
  const SqairTrackLogOut& o = *stitched;
  if (!o.track_id || !o.n_tracks || !o.len0 || !o.frame_index || !o.state || !o.size || !o.filt || !o.smooth)
    return sq_no(h, who + "stitched's track_id, n_tracks, len0, frame_index, state, size, filt and smooth must not be NULL");
  if (!stitch->link_next || !stitch->link_d2 || !stitch->link_gap || !stitch->root || !stitch->n_links)
    return sq_no(h, who + "link_next, link_d2, link_gap, root and n_links must not be NULL");
  const void* in[9] = {table->track_id, table->n_tracks, table->len0, table->frame_index, table->state, table->size, table->filt,
                       table->smooth, work};
  const void* out[9] = {o.track_id, o.n_tracks, o.len0, o.frame_index, o.state, o.size, o.filt, o.smooth, work_out};
  for (int i = 0; i < 9; ++i)
    for (int j = 0; j < 9; ++j)
      if (in[i] && in[i] == out[j]) return sq_no(h, who + "stitched and work_out must not share a pointer with table or work");
  LaneTrackLogStitchArgs a; memset(&a, 0, sizeof(a));
  a.log = *log; a.tab = *table; a.work = (const int32_t*)work; a.st = *stitch; a.out = o; a.work_out = (int32_t*)work_out;
  a.q = q; a.r = r; a.v0_var = v0_var; a.lag = lag; a.C = C; a.N = N; a.B = B;
  sq_launch_lane_tracklog_stitch(a, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
// trajectory scoring (include/sqair_hip.h: sqair_lane_traj_score): a stand-alone call on the table a lane forecast or a lane trace
// wrote -- or on a test's tensors --, nothing registered on the handle, which gives N and the error text
extern "C" int sqair_lane_traj_score(SqairHandle* h, const SqairLaneTraj* table, const SqairTrajTruth* truth, const SqairTrajScore* score,
                                     int F, int B, void* stream) {
  if (!h) return -1;
  const std::string who = "sqair_lane_traj_score: ";
  if (!table || !truth || !score) return sq_no(h, who + "table, truth and score must not be NULL");
  if (F < 1 || F > 65535 || B < 1) return sq_no(h, who + "F = " + std::to_string(F) + " must lie in 1..65535 and B = " + std::to_string(B) + " must be >= 1");
  if (sq_truth_slots_refusal(h, who, truth->G) != 0 || sq_unit_refusal(h, who, "iou_min", score->iou_min) != 0) return -1;
  if (!table->best_row || !table->presence || !table->support || !table->box0 || !table->alive || !table->box_mean || !table->count_prob)
    return sq_no(h, who + "the table's best_row, presence, support, box0, alive, box_mean and count_prob must not be NULL");
  if (!truth->anchor_box || !truth->anchor_present || !truth->anchor_valid || !truth->truth_box || !truth->truth_present || !truth->truth_valid)
    return sq_no(h, who + "anchor_box, anchor_present, anchor_valid, truth_box, truth_present and truth_valid must not be NULL");
  if (!score->counts || !score->sums || !score->lane_counts) return sq_no(h, who + "counts, sums and lane_counts must not be NULL");
  if (truth->keep_id && !table->obj_id) return sq_no(h, who + "keep_id needs the table's obj_id: the identities it is compared with");
  LaneTrajScoreArgs a; memset(&a, 0, sizeof(a));
  a.tab = *table; a.tr = *truth; a.sc = *score;
  a.F = F; a.B = B; a.N = h->cfg.n_steps_per_image; a.match = h->match_traj;
  sq_launch_lane_traj_score(a, (hipStream_t)stream);
  SQ_CHECK_HIP(hipGetLastError());
  return 0;
}
