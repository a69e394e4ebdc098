// Internal declarations shared by sqair_api.hip (handle, plan, forward pass), sqair_state.hip (carried state, forecast),
// sqair_lane_api.hip (lane answers), sqair_train.hip (backward pass), sqair_dense_test.hip and sqair_unit_test.hip (the unit-test entries).
#pragma once
#include <cstdio>
#include <cstring>
#include <map>

#include "sqair_dx.h"
#include "sqair_glue.h"
#include "sqair_pack.h"

struct ParamEntry {
  std::string name;
  int64_t off, numel;
  int rows, cols;
};

enum LayerId {
  L_IENC0, L_IENC1, L_PREDISC, L_PRIOR_GRU1, L_PRIOR_GRU2, L_PRIOR_LIN, L_TAU1, L_WB2, L_MASK2, L_GENC0, L_GENC1,
  L_WHAT_LOC, L_WHAT_HEAD, L_PRE, L_PROP_RNN, L_PROP_T1, L_PROP_T2, L_PROP_T3, L_PROP_GRU1, L_PROP_GRU2,
  L_PROP_HEADS, L_PROP_S1, L_LAT0, L_LAT1, L_PRED, L_RNCOND, L_DISC_RNN, L_DISC_T1, L_DISC_T2, L_DISC_T3,
  L_DISC_S1, L_DEC0, L_DEC1, L_DEC2, L_PROP_RNN2, L_DISC_RNN2,
  L_WHAT_HEAD_I, L_PROP_HEADS_I,   // forward-only packs with interleaved output columns (what fusion, sqair_glue.h: WhatArgs)
  L_COUNT
};

// The track history's ring as registered (sqair_set_history), by value: on the handle, and in the settings a pass resolves.
struct SqHistRing {
  bool on = false;
  void* ring = nullptr;
  int64_t bytes = 0;
  int L = 0;
  uint32_t fields = 0;
};
// The lane answers of a pass, by value: on the handle as registered, and in the settings a pass resolves (SqStateRes).  One
// launch each after the history push, before the resampler, in this order (sq_launch_lane_answers): the estimate
// (k_lane_estimate; T: the frames per pass its outputs were sized for), then its followers, which read what it writes and are
// only ever on with it and for its T -- the layers (k_lane_layers), the identity (k_lane_identity) and the score (k_lane_score).
// score_ids: the score reads the identity's lane_id for obj_id; only ever with both on.  idf: the IDF1 table (k_lane_idf), after the
// score and on the id words it was handed; only ever on with a score that binds truth_match.  hota: the HOTA clip log (k_lane_hota),
// after the score and the IDF on the same words; only ever on with a score.  tracklog: the track log (k_lane_tracklog), directly
// after the identity, whose lane_id and track_len it copies; only ever on with it.  All off is SqLaneSet{}.
struct SqLaneSet {
  bool est_on = false;
  SqairLaneEstimate est = {};
  int est_T = 0;
  bool lay_on = false;
  SqairLaneLayers lay = {};
  bool ident_on = false;
  SqairLaneIdentity ident = {};
  bool motion_on = false;          // sqair_set_motion: the identity's launch is its motion instantiation; only ever on with the identity
  SqairLaneMotion motion = {};
  bool tracklog_on = false;        // sqair_set_tracklog: k_lane_tracklog directly after the identity's node; only ever on with the identity
  SqairLaneTrackLog tracklog = {};
  bool score_on = false;
  SqairLaneScore score = {};
  bool score_ids = false;
  bool idf_on = false;
  SqairLaneIdf idf = {};
  bool hota_on = false;
  SqairLaneHota hota = {};
  // sqair_set_lane_match's score and identity, 0 = keep + greedy, 1 = keep + optimal: no registration -- the setting lives on the
  // handle (SqairHandle::match_*) and sq_resolve_pass copies it into the pass's resolved block, which is what the launches read
  int score_match = 0, ident_match = 0;
};

struct SqairHandle {
  // cfg is what the kernels run on: n_hidden rounded up to a width the row kernels are written for (a multiple of 128).  The extra
  // hidden units are inert by construction -- zero weights and biases in, zero weights out, zero initial states: ELU(0) = tanh(0)
  // = 0, a GRU / LSTM unit that starts at 0 with zero pre-activations stays at 0 -- so results equal the unpadded model's.  ucfg
  // is the caller's configuration.  `params` is the inventory in the PADDED shapes (everything downstream -- packing plan, POff,
  // the kernels that read small layers straight from the flat buffer -- sees only these); `uparams` is the caller's inventory
  // (reference shapes, what crosses the ABI) and u2i maps each of its elements to its place in the padded flat buffer.  When
  // nothing is padded (`padded` false: n_hidden 128 / 256 / ...) the two coincide and the caller's buffers are used as they are.
  SqairConfig cfg;
  SqairConfig ucfg;
  std::string err;
  std::vector<ParamEntry> params;
  std::map<std::string, int> pidx;
  int64_t n_params = 0;
  std::vector<ParamEntry> uparams;
  int64_t n_uparams = 0;
  std::vector<int> u2i;
  bool padded = false;
  POff po;
  // packing plan
  PackedLayer layers[L_COUNT];
  PackedLayer layersT[L_COUNT];     // transposed packs (dX = dY W^T), K' = padded N, N' = padded concat K
  // weight-gradient plan: per layer, one entry per (column block, segment) with the A-position -> matrix-row map
  struct WgEntry { int n0, ncols, col0, seg; std::string w; int64_t rm_off; };
  struct BgEntry { int n0, ncols, col0; std::string a, b; };
  std::vector<WgEntry> wg[L_COUNT];
  std::vector<BgEntry> bg[L_COUNT];
  std::vector<int> rm_pool;
  PackPlan plan;                    // index tables of layers[] then layersT[] (sqair_pack.h)
  bool plan_uploaded_to = false;
  const void* plan_uploaded_ptr = nullptr;
  // graph
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  int graph_nodes = 0;
  bool dense_log_on = false;           // sqair_debug_dense_log: {layer id, rows, K (padded to 16 per segment), N} of every dense launch
  std::vector<int> dense_log;          // of the passes issued while it was on (host side only: nothing changes on the device)
  bool opt_what_fusion = true;  // sqair_set_option("what_fusion"): the what sample of a slot inside the layer that produces its operands (bit-identical;
                                // taken while the layers it replaces run on the split-K kernel: sq_what_fusion, sqair_api.hip)
  bool opt_specialised = true;  // sqair_set_option("specialised"): the slot loop's per-row kernels in their instantiations for the shipped dimensions (bit-identical)
  int opt_specialised_mask = 3;    // sqair_set_option("specialised_mask"): which of them (SPEC_* bits, sqair_glue.h); a measurement aid
  bool opt_tail_fusion = true;  // sqair_set_option("tail_fusion"): the tail of slot k inside slot k + 1's RNN launch (bit-identical either way)
  bool opt_slot_chain = false;  // sqair_set_option("slot_chain"): the slot launches of a frame's propagation / discovery loop as one
                                // persistent launch each (sqair_chain.h; bit-identical; set BEFORE sizing / clearing workspaces)
  int opt_slot_chain_mode = 0;
  int opt_vi_target = 0;        // sqair_set_option("vi_target"): learning signal of sqair_elbo, 0 = VIMCO, 1 = plain REINFORCE
  void* chain = nullptr;        // ChainState (sqair_chain.hip)
  bool clear_each_pass = true;  // zero the caller's workspace at the start of every pass (sqair_set_workspace_clearing)
  const float* gen_noise = nullptr;  // sqair_set_generation_noise
  // carried model state (sqair_set_state): the following inference passes import it in the prologue / export it in the epilogue
  bool state_on = false;
  const void* state_in = nullptr;    // [R] rows of sq_state_row_floats(), or NULL = every row starts fresh
  void* state_out = nullptr;         // may equal state_in
  const int32_t* state_src = nullptr;  // [R] source row of each imported row (-1 = fresh), or NULL = identity
  int state_B = 0;
  // SMC resampling of the carried state (sqair_set_smc): one k_smc_resample launch after the state export
  bool smc_on = false;
  SqairSmc smc = {};                 // (smc.src_rows == state_src and its B == state_B while smc_on)
  // track history (sqair_set_history): one k_history_push launch after the state export, before the resampler
  SqHistRing hist;
  int hist_T = 0;                    // frames per pass of the ring's slots, 0 until the first pass pushes
  // missing-frame steps (sqair_set_observed): the passes' kernels read this device mask [observed_T][state_B]
  const int32_t* observed = nullptr;
  int observed_T = 0;
  // the lane answers (sqair_set_estimate / _layers / _identity / _motion / _tracklog / _score / _score_ids / _idf / _hota; sqair_lane_api.hip)
  SqLaneSet lane;
  // per-frame matching of the lane block (sqair_set_lane_match): a plain setting, untouched by the registrations above
  int match_score = 0, match_ident = 0, match_traj = 0;
  // generic capture slots (sqair_capture_begin / _end / _launch): any sequence of C-ABI calls as one HIP graph
  hipGraph_t cap_graph[4] = {nullptr, nullptr, nullptr, nullptr};
  hipGraphExec_t cap_exec[4] = {nullptr, nullptr, nullptr, nullptr};
};


inline int64_t align64(int64_t x) { return (x + 63) / 64 * 64; }
constexpr int64_t SQ_TRAIN_MAX_FRAME_BYTES = 150 * 1024;   // dynamic LDS the crop adjoint may ask for (sq_allow_big_lds)
int sq_state_refusal(SqairHandle* h, bool train, int B, int t_offset);   // -1 + error text: a pass a carried state rules out
// -1 + error text: a carried training call (sqair_forward_train_carry / sqair_backward_carry) that SqairCarry rules out; `out`
// (forward only, else NULL) is checked for the log weights SMC resamples on
int sq_carry_refusal(SqairHandle* h, const char* fn, int B, const SqairCarry* carry, const SqairOutputs* out);
bool sq_trainable_frame(SqairHandle* h);                   // false + error text when the handle's frames cannot be trained
int64_t P(const SqairHandle* h, const std::string& name);  // flat offset of a parameter (aborts on unknown names)
int PC(const SqairHandle* h, const std::string& name);      // its number of columns

// packed buffer = [weights fp32 | biases fp32 | widx int32 | bidx_a | bidx_b | row maps | (padded configurations only:) the flat
// parameters in the padded shapes fp32 | u2i int32], each 256-byte aligned
struct PackedLayout {
  int64_t w, b, wi, ba, bb, rm, fi, um, total;  // offsets in 4-byte words
};
inline PackedLayout packed_layout(const SqairHandle* h) {
  PackedLayout p;
  p.w = 0;
  p.b = align64(p.w + h->plan.packed_w());
  p.wi = align64(p.b + h->plan.packed_b());
  p.ba = align64(p.wi + h->plan.packed_w());
  p.bb = align64(p.ba + h->plan.packed_b());
  p.rm = align64(p.bb + h->plan.packed_b());
  p.fi = align64(p.rm + (int64_t)h->rm_pool.size());
  p.um = align64(p.fi + (h->padded ? h->n_params : 0));
  p.total = align64(p.um + (h->padded ? h->n_uparams : 0));
  return p;
}

struct Lin {
  LinArgs a;
  Lin() {
    memset(&a, 0, sizeof(a));
    a.epi = EPI_ACT;
    a.act_split = 1 << 30;
    a.add_rdiv = 1;
    a.scale = 1.0f;
  }
  Lin& seg(const float* p, int ld, int width, int rdiv = 1) {
    a.seg[a.nseg++] = LinSeg{p, ld, width, rdiv};
    return *this;
  }
  Lin& out(float* p, int ld) { a.out = p; a.out_ld = ld; return *this; }
  Lin& act(int act) { a.act_a = act; return *this; }
  Lin& act2(int a0, int a1, int split) { a.act_a = a0; a.act_b = a1; a.act_split = split; return *this; }
  Lin& add(const float* p, int ld, int n, int rdiv = 1) { a.add = p; a.add_ld = ld; a.add_n = n; a.add_rdiv = rdiv; return *this; }
  Lin& gru1(const float* hprev, int h_ld, float* rh, int rh_ld, float* xh, int xh_ld, int nh) {
    a.epi = EPI_GRU1; a.e0 = hprev; a.e0_ld = h_ld; a.o1 = rh; a.o1_ld = rh_ld; a.o2 = xh; a.o2_ld = xh_ld; a.nh = nh;
    return *this;
  }
  Lin& gru2(const float* hprev, int h_ld, const float* z, int z_ld, int nh) {
    a.epi = EPI_GRU2; a.e0 = hprev; a.e0_ld = h_ld; a.e1 = z; a.e1_ld = z_ld; a.nh = nh;
    return *this;
  }
};
// builder for the routed dX GEMM of layer `id` (sqair_dx.h): the backward's counterpart of Lin.  The forward names a layer's operands
// as segments; the reverse sweep names the same segments as destinations, and where segment i lies in the layer's padded K -- its
// start the earlier widths each rounded up to 16, its length the true width -- is derived here from the plan (sq_run_dx checks it).
struct SQ_LOCAL Dx {
  DxArgs a;
  LayerId id;
  const PackedLayer& L;
  static constexpr int MAXR = (int)(sizeof(DxArgs::r) / sizeof(DxRange));
  Dx(const SqairHandle* h, LayerId layer, const float* dpre, int ld) : id(layer), L(h->layers[layer]) {
    memset(&a, 0, sizeof(a));
    a.dpre = dpre; a.ld = ld; a.width = L.N;
  }
  DxRange& last() { return a.r[(a.nranges < MAXR ? a.nranges : MAXR) - 1]; }
  // segment i of the layer -> dst (an i the layer does not have, or one range too many: refused by sq_run_dx)
  Dx& seg(int i, float* dst, int dst_ld) {
    if (a.nranges++ >= MAXR) return *this;
    const int nseg = (int)L.seg_width.size();
    DxRange& r = last();
    for (int j = 0; j < i && j < nseg; ++j) r.n0 += (L.seg_width[j] + 15) / 16 * 16;
    r.n1 = r.n0 + (i >= 0 && i < nseg ? L.seg_width[i] : 0); r.dst = dst; r.dst_ld = dst_ld; r.act_split = 1 << 30;
    return *this;
  }
  Dx& acc() { last().add = last().dst; last().add_ld = last().dst_ld; return *this; }
  Dx& add(const float* p, int ld) { last().add = p; last().add_ld = ld; return *this; }
  Dx& dact(const float* saved, int ld, int act_a, int act_b = ACT_NONE, int split = 1 << 30) {
    last().saved = saved; last().saved_ld = ld; last().act_a = act_a; last().act_b = act_b; last().act_split = split;
    return *this;
  }
  Dx& dup(float* p, int ld) { last().dst2 = p; last().dst2_ld = ld; return *this; }
  // GRU gate adjoints in this launch's epilogue (DxGru): mode 1 = after the d h' GEMM, mode 2 = after the d(r h) GEMM
  Dx& gru_a(const float* z, int z_ld, const float* hc, int hc_ld, const float* hprev, int h_ld, float* dpre1, int dp_ld, float* d_h,
            int dh_ld, int acc_dh, int nh, float* dupp = nullptr, int dup_ld = 0, int dup_h_off = -1) {
    a.gru = DxGru{1, z, z_ld, hc, hc_ld, hprev, h_ld, dpre1, dp_ld, d_h, dh_ld, acc_dh, dupp, dup_ld, dup_h_off, nh};
    return *this;
  }
  Dx& gru_b(const float* r, int r_ld, const float* hprev, int h_ld, float* dpre1, int dp_ld, float* d_h, int dh_ld, int nh,
            float* dupp = nullptr, int dup_ld = 0) {
    a.gru = DxGru{2, r, r_ld, nullptr, 0, hprev, h_ld, dpre1, dp_ld, d_h, dh_ld, 1, dupp, dup_ld, -1, nh};
    return *this;
  }
};



// ------------------------------------------------------------------------------------------------
// workspace.  In training mode (train = true) every intermediate the backward pass needs is kept: per-frame
// buffers become [T][...], per-slot buffers a "tape" [2 phases][T][B'][N slots][width] (slot-inner like the slot
// records, so a slot launch addresses it with row stride N * width and the batched weight-gradient GEMMs see all
// uses of a layer as one long row range).
// ------------------------------------------------------------------------------------------------
// leading dimensions of the activation buffers: room for the widest layer the build accepts (prior statistics 2 (4 + n_what) + 1,
// glimpse-encoder Gaussian 2 n_what, loc1 n_what, raw heads 5 n_what, transform hidden | steps hidden 1.5 n_hidden, steps hidden
// n_hidden / 2), each a multiple of 16
#ifdef SQAIR_WIDE
constexpr int PS_LD = 272, ENC_LD = 256, M1_LD = 128, HRAW_LD = 640, WB_LD = 4, TP_LD = 8, T1_LD = 768, S1_LD = 256;
#else
constexpr int PS_LD = 112, ENC_LD = 112, M1_LD = 64, HRAW_LD = 256, WB_LD = 4, TP_LD = 8, T1_LD = 384, S1_LD = 128;
#endif

// row of (frame t, phase ph, slot k) in a slot tape [phase][T][B'][N]: the one index formula of the workspace's tapes
// (Workspace::slot) and of the backward's mirrors of them (BwdSpace::slot, sqair_train.hip)
inline size_t sq_tape_row(int T, int R, int N, int t, int ph, int k) { return (size_t)(ph * T + t) * R * N + k; }
struct Workspace {
  bool train;
  bool tape;    // per-frame / per-slot buffers are kept apart ([T] / [2 phases][T][B'][N]): training, or the in-launch slot chain
  bool chain;   // the slot loops run as chain launches (sqair_chain.h)
  unsigned* chain_ctl;   // control blocks of the pass's chain launches
  int T, B, R, M, N, nh, snh, psnh, G2, pgw;   // (pgw: width of the prior cell's kept gates pgz)
  float *ienc_a, *ienc_b, *pre_disc;
  float *rec_m_all, *rec_p_all, *rec_d_all;
  float *temporal_m, *prior_m;                   // train: [T+1][M][snh | nh], else [2][M][snh | nh]
  float *last_id[2];
  float *zero_rec, *disc_init_rec, *prop_rnn_init, *disc_rnn_init, *rn_init_state, *w3_prop, *w3_disc;
  float *temporal_p, *prior_p;                   // per frame
  float *pgz, *pgr, *pghc, *pgrh, *pgxh;         // prior GRU internals, per frame
  float *pstats, *spre;                          // always [T]
  float *hid1, *wb, *mask, *g1, *pea, *peb, *m1, *pre, *lea, *leb, *c, *pre_d;  // per frame
  float *r, *t1, *t2, *tp, *g2, *e1, *e2, *enc, *hraw, *s1h, *gz, *gr, *ghc, *grh, *gxh;  // per slot
  float *rc, *rgates;                            // LSTM / GRU slot RNN: cell states (like r), kept gates [.][4nh | 3nh]
  float *lpre, *lgates;                          // LSTM temporal cell (time_lstm): [M][4nh], kept gates [T][R][N][4nh]
  int* src;                                      // train: compaction source slot [T][R][N]
  float *qz, *pz, *dlp, *dll, *glimpse, *dec_a, *dec_b;
  float* gen;                                    // sample_from_prior: [T][M][64] prior samples + original presences
  float* obs_p;                                  // frames whose H * W is not a multiple of 4: zero-padded copy [T*B][P4] (else unused)
  int* t_row;                                    // carried state: frame counter of each row at frame 0 of the pass [R]
  float* fresh;                                  // train: 1 / 0 per row slot [R][N], fresh / imported row (k_state_import)
  int64_t clear_n;  // floats from the base that a workspace clear covers: every buffer carved before chain_ctl
  int64_t total;    // floats

  float* frame(float* base, int64_t per_frame, int t) const { return base + (tape ? (size_t)t * per_frame : 0); }
  float* state(float* base, int t, int width) const { return base + (size_t)(tape ? t : (t & 1)) * M * width; }
  // What both passes address of frame t: the records, the merged states on either side of it, and the per-frame buffers.  at() is the
  // only caller of frame(): it stands beside sq_carve (sqair_api.hip), each stride against the take() that sized its buffer.
  struct Frame {
    float *rec_prev, *rec_next, *rec_p, *rec_d, *pstats, *spre;
    float *temporal_prev, *temporal_next, *prior_prev, *prior_next, *temporal_p, *prior_p;
    float *pgz, *pgr, *pghc;
    float *hid1, *wb, *mask, *g1, *pea, *peb, *m1, *lea, *leb, *c;
  };
  SQ_LOCAL Frame at(int t) const;
  // slot buffer of width W: pointer of (frame t, phase ph, slot k) and its row stride
  float* slot(float* base, int W, int t, int ph, int k) const { return base + (tape ? sq_tape_row(T, R, N, t, ph, k) * W : 0); }
  int sld(int W) const { return tape ? N * W : W; }
  float* cslot(int t, int ph, int k) const { return tape ? slot(rc, nh, t, ph, k) : rc + (size_t)(k & 1) * R * nh; }
  float* rslot(int t, int ph, int k) const {  // RNN hidden state: ping-pong over slots when no tape is kept
    return tape ? slot(r, nh, t, ph, k) : r + (size_t)(k & 1) * R * nh;
  }
};
Workspace sq_carve(const SqairHandle* h, int T, int B, float* base, bool train);

// (sq_no, a refusal: -1 + error text, stands beside sq_set_error in sqair_common.h)
static inline int sq_refuse(SqairHandle* h, const char* who, const std::string& why) { return sq_no(h, std::string(who) + ": " + why); }
// -1 + "<who><name> must lie in (0, 1]" unless it does: an IoU or coverage threshold (NaN fails both comparisons)
static inline int sq_unit_refusal(SqairHandle* h, const std::string& who, const char* name, float v) {
  return v > 0.0f && v <= 1.0f ? 0 : sq_no(h, who + name + " must lie in (0, 1]");
}

// ---- carried model state (sqair_state.hip) ----
int64_t sq_state_row_floats(const SqairHandle* h);   // floats of one particle row of the state blob
// The carried-state settings of one pass, resolved once per call and passed by value: the handle's (sq_resolve_pass; all off for
// a training pass) or a carried training call's (sq_carry_state).  The pass and the argument builders it calls read these, never
// the handle's registration fields (of the handle only cfg and the error text), and nothing between resolution and return writes
// those.  `fresh`: k_state_import records each row's fresh / imported flag for the backward.  hist, observed and lane: the
// handle's inference passes only -- a carried training call never pushes, coasts on the handle's mask or answers per lane.
struct SqStateRes {
  bool on = false;
  const void* in = nullptr;
  void* out = nullptr;
  const int32_t* src = nullptr;
  bool fresh = false;
  bool smc_on = false;
  SqairSmc smc = {};
  const int32_t* observed = nullptr;   // (the handle's device mask of sqair_set_observed, a masked carried chunk's own, or NULL)
  SqHistRing hist;
  SqLaneSet lane;
};
// The refusals of a pass on the handle's settings -- observed mask, state, SMC, history, estimate, in this order (-1 + error text,
// before any HIP call) -- then the settings in *st.  The only place that fixes the history ring's T: a refused call changes nothing.
SQ_LOCAL int sq_resolve_pass(SqairHandle* h, bool train, int T, int B, int t_offset, const SqairOutputs* out, SqStateRes* st);
// `st` for a pass that changes nothing outside its workspace and outputs (a capture's eager pre-pass): what it reads stays (the rows
// imported through the map, the mask), what it writes goes (export, history push, the lane answers, resampler).
SQ_LOCAL SqStateRes sq_without_effects(SqStateRes st);
SQ_LOCAL SqStateRes sq_carry_state(const SqairCarry* c);
SQ_LOCAL StateArgs sq_state_args(const SqairHandle* h, const SqStateRes& st, int R, float* rec, float* temporal, float* prior, float* last_id,
                                 int* t_row, float* fresh, int t0);
// -1 + "<who>B = ... but the state ..." when a call's B is not the registered state's
SQ_LOCAL int sq_state_b_mismatch(SqairHandle* h, const std::string& who, int B);
// missing-frame steps: -1 + error text for a training call, or a pass of another T, while a mask is set (host only)
SQ_LOCAL int sq_observed_refusal(SqairHandle* h, bool train, int T);
// track history: the push's arguments for a pass of T frames into the ring of `st` (of `h` only cfg)
SQ_LOCAL HistPushArgs sq_history_push_args(const SqairHandle* h, const SqStateRes& st, const SqairOutputs& out, const int* t_row, int T, int B);
SQ_LOCAL SmcArgs sq_smc_args(const SqairSmc& m, const float* lw, const int32_t* t_row, int T, int B, int K);
// ---- lane answers (sqair_lane_api.hip) ----
// the refusal of a pass with the estimate on (host only: before any HIP call; sq_resolve_pass calls it last)
SQ_LOCAL int sq_estimate_refusal(SqairHandle* h, int T, const SqairOutputs* outp);
// The lane launches of a pass of T frames, `l` as resolved: estimate -> layers -> identity -> track log -> score -> IDF -> HOTA over the merged records `rec`
// [T][R][N][rec::W], the decoded glimpses `glimpse` [T][R][N][G*G] and the pass's outputs.  0, or -2 + error text when the layers'
// launch fails (dynamic LDS limit).  Of `h` only cfg and the error text.
SQ_LOCAL int sq_launch_lane_answers(SqairHandle* h, const SqLaneSet& l, const float* rec, const float* glimpse, const SqairOutputs& out,
                                    int T, int B, hipStream_t s);
// ---- the slot step's argument builders and launch helpers (sqair_api.hip), shared by the pass and by the forward unit entries
// (sqair_slot_crop_test, sqair_slot_tail_test, sqair_linear_what_test: sqair_unit_test.hip) ----
// What a slot's tail takes from its caller; sq_tail_args adds what the handle resolves (the *_S1 pack, the steps.l1 offsets).
struct TailOperands {
  int is_disc, slot, what_done;
  const float* hraw; int h_ld;
  const float* enc; int enc_ld;
  const float* rec_prev; float* rec_new;
  const float* noise;
  const float* s1p; int s1p_ld;
  float* s1h_out; int s1h_ld;
};
// What a crop of the slot loop takes from its caller (the fields of CropArgs, sqair_glue.h); sq_crop_args keeps what the mode reads.
struct CropOperands {
  int mode, slot;
  const float* img;
  const float* mask; int mask_row_mul, mask_row_add;
  float* out; int out_row_mul, out_row_add;
  const float* rec_prev; float* rec_new;
  const float* wb; int wb_ld;
  const float* tp; int tp_ld;
  const float* t2; int t2_ld;
  const float* w3;
  const float* noise; const float* flat;
  float* tp_out; int tp_out_ld;
};
SQ_LOCAL CropArgs sq_crop_args(const CropOperands& o);
SQ_LOCAL int sq_crop_slots(int mode, const Dims& d);
SQ_LOCAL Dims sq_pass_dims(const SqairHandle* h, int B, int spec_mask);
SQ_LOCAL TailArgs sq_tail_args(const SqairHandle* h, const TailOperands& io, const float* flat, const float* packed);
// the tail of slot ta.slot can ride in the next slot's VanillaRNN layer `id` (L_PROP_RNN / L_DISC_RNN): k_rnn_tail serves it
SQ_LOCAL bool sq_can_fuse_tail(const SqairHandle* h, LayerId id);
SQ_LOCAL int sq_run_rnn_tail(SqairHandle* h, const TailArgs& ta, Dims d, LayerId id, const float* hid, int hid_ld, const float* add, int add_ld,
                             float* out, int out_ld, const float* packed, hipStream_t s);
// k_linear_what on the handle's L_WHAT_HEAD_I (mode 0) / L_PROP_HEADS_I (mode 1) pack
SQ_LOCAL int sq_run_what(SqairHandle* h, int mode, const float* x, int x_ld, int M, int slot, const float* noise, const float* enc, int enc_ld,
                         const float* rec_prev, float* rec_new, const float* packed, hipStream_t s);
// what the training pass shares with the adjoint unit entries (sqair_train.hip), beside sq_pass_dims(h, B, 0), the Dims of a training
// pass over B sequences: the steps predictor's offsets a slot-tail adjoint reads
struct TailBwdArgs;
SQ_LOCAL void sq_tail_param_offsets(const SqairHandle* h, bool is_disc, TailBwdArgs* ta);
// section A of a frame of the pass, and a frame of the forecast: the propagation-prior cell and its statistics (sqair_api.hip)
SQ_LOCAL int sq_prior_step(SqairHandle* h, const float* packed, hipStream_t s, int M, const float* rec_prev, const float* prior_prev,
                           float* prior_p, float* pgz, float* pgrh, float* pgxh, float* pstats, float* o3, float* o1);

// Capture on this stream, scoped: on every way out that did not hand_over() the graph and its executable, the destructor ends a
// capture still open (a stream left capturing fails every later call on it) and destroys what was made, the two timing events of
// the measurement helpers included.  (sqair_capture_begin / _end are paired by the caller and do not use this.)
struct SqCapture {
  hipStream_t s;
  bool open = false;
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  explicit SqCapture(hipStream_t stream) : s(stream) {}
  SqCapture(const SqCapture&) = delete;
  hipError_t begin() { const hipError_t e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal); open = e == hipSuccess; return e; }
  hipError_t end() { open = false; return hipStreamEndCapture(s, &graph); }
  hipError_t instantiate() { return hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0); }
  hipError_t events() { const hipError_t e = hipEventCreate(&ev[0]); return e != hipSuccess ? e : hipEventCreate(&ev[1]); }
  void hand_over(hipGraph_t* g, hipGraphExec_t* x) { *g = graph; *x = exec; graph = nullptr; exec = nullptr; }
  ~SqCapture() {
    if (open) (void)hipStreamEndCapture(s, &graph);
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
  }
};

// zero fill as a kernel (not a memset node: see sqair_train.hip); p 16-byte aligned
void sq_zero_fill(float* p, int64_t n, hipStream_t s);
void sq_copy(float* dst, const float* src, int64_t n, hipStream_t s);

// the flat parameter buffer the kernels read: the caller's, or (padded configurations) the padded copy sqair_pack_params keeps
// inside the packed buffer
inline const float* sq_flat(const SqairHandle* h, const float* user_flat, const void* packed) {
  return h->padded ? (const float*)packed + packed_layout(h).fi : user_flat;
}
void sq_flat_gather(const SqairHandle* h, const float* padded_grad, float* user_grad, const void* packed, hipStream_t s);
int sq_run(SqairHandle* h, Lin& l, LayerId id, int M, const float* packed, hipStream_t s);
// the routed dX GEMM of x's layer over M rows; refuses what sq_run refuses, -3 + "internal: ... in dX of layer <id>", before the launch
SQ_LOCAL int sq_run_dx(SqairHandle* h, Dx& x, int M, const float* packed, hipStream_t s, const float* scale_ptr = nullptr);
#define RUN(l, id, M)                                   \
  do {                                                  \
    int _rc = sq_run(h, (l), (id), (M), packed, s);     \
    if (_rc != 0) return _rc;                           \
  } while (0)
