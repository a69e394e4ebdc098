// Launchers of the non-GEMM kernels (sqair_glue.hip; the kernels of the per-lane answers: sqair_lane.hip).
#pragma once
#include "sqair_common.h"

// Limits of a build.  The product library is laid out for the shipped model family (slot record with 50 `what` entries, 8 slots,
// hidden layers up to 256 wide); libsqair_hip_wide.so is the same source compiled with -DSQAIR_WIDE for the rest of the range the
// reference's flags span: larger records, more slots, wider layers -- slower kernels (more registers / LDS per workgroup), same
// results, same C-ABI.  sqair_amd picks the library from the flags.
#ifdef SQAIR_WIDE
constexpr int SQ_MAXN = 16;          // n_steps_per_image
constexpr int SQ_MAX_NWHAT = 128;    // n_what
constexpr int SQ_MAX_NHIDDEN = 512;  // 32 * n_units (after padding to a multiple of 128)
#else
constexpr int SQ_MAXN = 8;           // max object slots supported by the small per-row kernels
constexpr int SQ_MAX_NWHAT = 50;
constexpr int SQ_MAX_NHIDDEN = 256;
#endif
constexpr int SQ_MAX_K = 256;        // k_particles

// Offsets (in floats) into the flat parameter buffer of the small layers the per-row kernels read
// straight from the unpacked parameters.
struct POff {
  int dec_mean_img, dec_output_scale;
  int rn_init_state, rn_init_sample, rn_readout_w, rn_readout_b, rn_cond_w, rn_cond_b, rn_h2h_w, rn_h2h_b,
      rn_i2h_w, rn_i2h_b;
  int sp_l0_w, sp_l0_b, sp_l1_w, sp_l1_b, step_prior_bias, step_prior_tbias;
  int disc_steps_l1_w, disc_steps_l1_b, prop_steps_l1_w, prop_steps_l1_b;
  int disc_scale_offset, prop_scale_offset, cholesky;
  int disc_rnn_init, prop_rnn_init, prior_init, temporal_init;
};

// floor(e / x) == __umulhi(e, mul) + (e & one) for 0 <= e < 2^32 / x with mul = floor(2^32 / x) + 1, one = 0; x = 1 (whose
// multiplier does not fit 32 bits): mul = 0, one = all ones.  No select, no branch.
struct SqMagic { unsigned mul, one; };
inline SqMagic sq_magic(int x) { return x <= 1 ? SqMagic{0u, 0xffffffffu} : SqMagic{(unsigned)((1ull << 32) / (unsigned)x + 1), 0u}; }
struct Dims {
  int H, W, G, N, nw, nh, K, R, B;  // R = B*K rows
  int nzw;                          // noise width = 4 + nw + 1
  int snh;                          // width of the temporal state of a slot: nh (GRU) or 2 nh = [hidden | cell] (LSTM)
  int toff;                         // offset of the features the model reads from it: 0 (GRU state) / nh (LSTM cell, core.py:284)
  int psnh;                         // width of the propagation prior's recurrent state: nh (GRU) or 2 nh (LSTM)
  int rsnh;                         // width of the slot RNN's trainable initial state: nh (VanillaRNN) or 2 nh (LSTM)
  SqMagic nw_mul, g_mul, k_mul;     // sq_magic(nw), sq_magic(G), sq_magic(K): e / x == sq_div(e, x_mul).  A runtime integer division is
                                    // ~25 instructions; in the slot tail and the crops it stood ahead of the operand loads of every
                                    // launch of the slot loop (forward step 3.44 -> 3.39 ms, training 7.90 -> 7.84)
  int P4;                           // floats between consecutive frames in the buffer the kernels read frames from: H * W, or --
                                    // inside a pass over frames whose H * W is not a multiple of 4 -- H * W rounded up to 4 (the
                                    // pass stages such frames through a zero-padded copy so that every frame starts 16-byte aligned)
  int spec;                         // which of the slot loop's kernels the pass launches in their specialised instantiations (SPEC_* bits;
                                    // sq_spec_ok below and sqair_set_option("specialised")); set by the forward pass, 0 everywhere else
};
// Specialised instantiations of the slot loop's crops and of the compaction (k_crop_row, k_compact).  These launches are
// hops of a chain of dependent launches whose length is the instruction stream of their longest wave, and much
// of that stream is arithmetic on values the host knows: the dimensions of the shipped model family and the mode of the launch.  When a handle's dimensions are the ones below, the launchers pick an instantiation that has them as
// compile-time constants (Dims replaced by sq_spec_dims inside the kernel, the mode a template argument): same expressions in the
// same order on the same operands, so the results are bit-identical to the generic instantiation, which serves everything else.
namespace spec {
constexpr int H = 50, W = 50, G = 20, N = 4, NW = 50, NH = 256;
}
inline bool sq_spec_ok(const Dims& d) {
#ifdef SQAIR_WIDE
  (void)d;
  return false;   // (the wide build keeps its plain-loop kernels)
#else
  return d.H == spec::H && d.W == spec::W && d.G == spec::G && d.N == spec::N && d.nw == spec::NW && d.nh == spec::NH &&
         d.nzw == 4 + spec::NW + 1 && d.snh == spec::NH && d.toff == 0 && d.psnh == spec::NH && d.P4 == spec::H * spec::W;
#endif
}
// Which kernels take their specialised instantiation is a mask in Dims::spec, all of them by default: with one bit set
// (sqair_set_option("specialised_mask")) each of them is timed, or checked for equal bits, on its own inside ONE binary -- two builds
// that differ in the set of kernels they contain differ by +-0.03 ms per cfg-2 step from code placement alone.
enum { SPEC_CROP = 1, SPEC_COMPACT = 2, SPEC_ALL = 3 };
// launches of specialised instantiations issued (or captured) by this process so far: a debug query for the tests
long long sq_spec_launches();
void sq_spec_count(int n);
#ifdef __HIPCC__
__device__ __forceinline__ int sq_div(int e, SqMagic m) { return (int)(__umulhi((unsigned)e, m.mul) + ((unsigned)e & m.one)); }
#endif
enum { RNN_VANILLA = 0, RNN_LSTM = 1, RNN_GRU = 2 };    // SqairConfig.rnn_cell (flag transition)
enum { CELL_GRU = 0, CELL_LSTM = 1, CELL_VANILLA = 2 };  // SqairConfig.time_cell / .prior_cell (flags time_transition / prior_transition)
// pre-activation columns of the slot RNN: nh (VanillaRNN), the four LSTM gates, or the GRU's [z | r | candidate]
inline int sq_rnn_width(const SqairConfig& c) { return c.n_hidden * (c.rnn_cell == RNN_LSTM ? 4 : (c.rnn_cell == RNN_GRU ? 3 : 1)); }
// gate pre-activation columns of the temporal / prior cell: 3 nh (GRU: z, r, candidate), 4 nh (LSTM), nh (VanillaRNN)
inline int sq_gate_width(const SqairConfig& c, int cell) { return c.n_hidden * (cell == CELL_LSTM ? 4 : (cell == CELL_VANILLA ? 1 : 3)); }
inline Dims make_dims(const SqairConfig& c, int B) {
  const bool lstm = c.time_cell == CELL_LSTM;
  return Dims{c.img_h, c.img_w, c.glimpse_size, c.n_steps_per_image, c.n_what, c.n_hidden, c.k_particles, B * c.k_particles, B,
              4 + c.n_what + 1, lstm ? 2 * c.n_hidden : c.n_hidden, lstm ? c.n_hidden : 0,
              (c.prior_cell == CELL_LSTM) ? 2 * c.n_hidden : c.n_hidden, c.rnn_cell == RNN_LSTM ? 2 * c.n_hidden : c.n_hidden,
              sq_magic(c.n_what), sq_magic(c.glimpse_size), sq_magic(c.k_particles), c.img_h * c.img_w, 0};
}

#ifdef __HIPCC__
// Dims of a specialised instantiation: what sq_spec_ok has checked becomes a constant, the rest (R, B, K and its multiplier) stays
template <int X> constexpr SqMagic sq_magic_c() { return SqMagic{(unsigned)((1ull << 32) / (unsigned)X + 1), 0u}; }
template <bool SP>
__device__ __forceinline__ Dims sq_spec_dims(const Dims& d) {
  if (!SP) return d;
  Dims c = d;
  c.H = spec::H; c.W = spec::W; c.G = spec::G; c.N = spec::N; c.nw = spec::NW; c.nh = spec::NH; c.nzw = 4 + spec::NW + 1;
  c.snh = spec::NH; c.toff = 0; c.psnh = spec::NH; c.P4 = spec::H * spec::W;
  c.nw_mul = sq_magic_c<spec::NW>(); c.g_mul = sq_magic_c<spec::G>();
  return c;
}
// Particle row handled by workgroup i of a launch with one workgroup per row (grid.x = R, R a multiple of 8).  Workgroups go to
// the eight XCDs round-robin (XCD = i % 8), each XCD has its own L2, and the K particles of a sequence read the SAME frame: with
// rows taken in launch order a frame was fetched into up to K of the eight L2s (PMC: 2.5x the algorithmic bytes of k_crop_row).
// With the number of sequences a multiple of 8, sequence b's K rows go to XCD b % 8, so a frame enters one L2.
__device__ __forceinline__ int sq_row_of_wg(int i, const Dims& d) {
  if ((d.B & 7) != 0) return i;
  const int xcd = i & 7, j = i >> 3;
  const int bb = sq_div(j, d.k_mul), k = j - bb * d.K;
  // (wave-uniform by construction; said so explicitly: the multiply-high of sq_div is a vector instruction, and a row index in a
  // VGPR turns every address of the kernel into vector arithmetic)
  return __builtin_amdgcn_readfirstlane((bb * 8 + xcd) * d.K + k);
}
#endif
enum CropMode { CROP_PLAIN = 0, CROP_PROP1 = 1, CROP_PROP2 = 2, CROP_DISC = 3 };
// Frames up to this many pixels are staged in LDS by the crop kernels while the where computation runs (a 50 x 50 frame is
// 10 KB: the copy hides behind the where sample); larger ones (BASELINE configs[4]: 128 x 128 = 64 KB per workgroup, of which a
// 20 x 20 glimpse touches at most 1600 pixels) are sampled where they lie -- four taps per glimpse pixel straight from L2, all
// in flight at once, instead of 54 dependent copy trips per thread
constexpr int SQ_CROP_STAGE_MAX_PIXELS = 4096;

struct CropArgs {
  int mode;
  const float* img;        // [B,H,W] frame t
  const float* logits;     // PLAIN: [R,4]
  const float* mask;       // optional [rows, G*G]
  int mask_row_mul, mask_row_add;  // mask row = r*mul + add
  float* out;              // [rows, G*G]
  int out_row_mul, out_row_add;
  const float* rec_prev;   // merged records of t-1 [R,N,168]
  float* rec_new;          // prop / disc records of this frame [R,N,168]
  const float* wb;         // PROP1: raw where-bias MLP output [(R*N), wb_ld]
  int wb_ld;
  const float* tp;         // PROP2 / DISC: transform MLP output [R, tp_ld] (loc 0:4, raw scale 4:8), or
  int tp_ld;
  const float* t2;         // ... its input [R, t2_ld]: the 256 -> 8 output layer is then evaluated in this launch
  int t2_ld;
  const float* w3;         // 16-byte aligned copy of transform.l2 {w [nh,8], b [8]} (workspace, see k_init_state)
  const float* noise;      // noise of frame t, [R,2,N,nzw]
  const float* flat;       // flat parameters
  int slot;                // PROP2 / DISC slot; PROP1 uses blockIdx.y
  float* tp_out;           // optional (training): the transform output [R, tp_out_ld] (loc 0:4, raw scale 4:8)
  int tp_out_ld;
};

int sq_launch_lstm_cell2(const float* gates, int g_ld, const float* c_prev, int c_ld, float* h_out, int h_ld, float* c_out, int co_ld,
                         int rows, int nh, hipStream_t s);
int sq_launch_lstm_cell(const float* gates, int g_ld, const float* c_prev, int c_ld, float* state_out, int o_ld, int rows, int nh,
                        hipStream_t s);
int sq_launch_init_state(float* rec_m, float* temporal_m, float* prior_m, float* last_id, float* disc_init_rec,
                         float* prop_rnn_init, float* disc_rnn_init, float* rn_init_state, float* w3_prop, float* w3_disc,
                         int w3p_off, int w3d_off, const float* flat,
                         POff po, Dims d, hipStream_t s);
int sq_launch_crop(const CropArgs& a, POff po, Dims d, int nslots, hipStream_t s);
// Tail of a propagation / discovery slot in one launch: what-sample, the what-dependent part of the steps
// predictor's hidden layer (small MFMA, K = 56), its output layer (dot with w2) and the presence Bernoulli.
struct TailArgs {
  int is_disc, slot;
  const float* hraw; int h_ld;      // prop: raw what-head (2 nw) + gate (3 nw) pre-activations
  const float* enc; int enc_ld;     // glimpse-encoder Gaussian (loc nw | scale nw)
  const float* rec_prev;            // merged records of t-1
  float* rec_new;                   // rec_p / rec_d
  const float* noise;               // noise of frame t
  const float* s1p; int s1p_ld;     // [R, nh/2] hidden pre-activation without the `what` term
  const float* wp;                  // packed [nh/32 ... ] weights of the `what` rows of steps.l0 (layer *_S1)
  const float* flat; int w2_off, b2_off;
  float* s1h_out; int s1h_ld;       // optional (training): the hidden activations elu(.) [R, nh/2]
  int what_done;                    // 1: the slot's what sample (what, what_loc, what_scale of rec_new) has been written by the layer that
                                    // produces its operands (k_linear_what below): the tail reads `what` instead of deriving it
};
// "What fusion" (round 6; INFERENCE passes only -- in a training pass the layer would also have to write its own output to the tape for
// the adjoint, in the reference column order: measured, 7.34 -> 7.38 ms per training step, against 7.35 without the fusion there): the what sample of a slot computed in the epilogue of the dense layer that
// produces its last operands -- a discovery slot's in the glimpse encoder's Gaussian head (what = loc + scale eps,
// sqair/core.py:226-229), a propagation slot's in the temporal cell's heads (the gated mixture of sqair/core.py:336-359) --
// through packs whose output columns put the two / five pre-activations of one `what` element into adjacent lanes
// (L_WHAT_HEAD_I, L_PROP_HEADS_I).  The element-wise work is then done ONCE per element by the lanes of one launch instead of
// by every one of the 16 column-tile workgroups of the next slot's fused RNN + tail launch, whose per-workgroup instruction
// stream is what that launch waits for (timing ablation: -2.8 % of the cfg-2 forward step).  Same arithmetic on the same
// operands: results are bit-identical to the tail deriving the sample from the plain layer's output AS LONG AS THAT LAYER RUNS ON THE
// SPLIT-K KERNEL (k_linear_what is its GEMM: four per-wave partial sums, reduced in wave order).  The pass therefore takes the
// fusion only below the row count at which sq_launch_linear hands the plain layers to the throughput kernels, which sum the K
// chunks in sequence (sq_linear_leaves_split_k: 6000 rows; sq_what_fusion, sqair_api.hip; tests/test_hip_forward.py,
// tests/test_slot_forward_kernels.py).
struct WhatArgs {
  int mode;                          // 0: discovery (pairs loc, scale); 1: propagation (t_loc, t_scale, forget, input, temporal gate)
  const float* x; int x_ld;          // A operand [M][K = 16 kc] (one segment, 16-byte aligned rows)
  const float* wp; const float* wzero; const float* bias;   // interleaved pack of the layer, the packed buffer's zero block, packed bias
  int M, kc, n_tiles, nw, N, slot, nzw;
  const float* noise;                // noise of frame t [R][2][N][nzw]
  const float* enc; int enc_ld;      // mode 1: glimpse-encoder Gaussian of the slot [R][loc nw | scale nw]
  const float* rec_prev;             // mode 1: merged records of t - 1 [R][N][rec::W]
  float* rec_new;                    // rec_p / rec_d of this frame: what, what_loc, what_scale of (row, slot) are written
  int layer_id;                      // (for the host-side launch log)
};
int sq_launch_linear_what(const WhatArgs& a, hipStream_t s);
int sq_launch_slot_tail(const TailArgs& a, Dims d, hipStream_t s);
int sq_launch_rnn_tail(const TailArgs& ta, Dims d, const float* hid, int hid_ld, const float* wp, const float* bias, const float* add,
                       int add_ld, float* out, int out_ld, int n_out, hipStream_t s);
int sq_launch_latent_sum(const float* f, const float* rec_p, float* c, Dims d, hipStream_t s);

struct LogprobArgs {
  const float* rec_p; const float* rec_d; const float* rec_prev;
  const float* pstats; int ps_ld;     // raw prior linear output [(R*N), ps_ld]
  const float* spre;                  // [R,128] pre-activation of the where-prior conditioning state (without e)
  const float* flat;
  int t_global;                       // absolute frame index (categorical prior is time dependent)
  const int* t_row;                   // carried state: absolute index of frame 0 per row [R] (replaces t_global), or NULL
  int t;                              // index of the first frame inside the output tensors
  int n_frames;                       // frames covered by the launch (inputs are [n_frames][...] contiguous)
  float* qz; float* pz; float* disc_lp;  // frame scalars [R]
  const float* gen;                   // sample_from_prior: generation records [n_frames][R*N][64] (see GenArgs), else NULL
  SqairOutputs out;
  SqairConfig cfg;
};
int sq_launch_logprob(const LogprobArgs& a, POff po, Dims d, hipStream_t s);
size_t sq_logprob_lds_bytes(const Dims& d, int ps_ld);   // k_logprob's dynamic LDS at a pstats pitch: what it stages per row

// Carried model state (sqair_set_state).  One blob row per particle row r, 32-bit words:
//   [N * rec::W slot records | N * snh temporal state | N * psnh prior state | last_id | frame counter (int32) | zero padding]
// in the kernels' own (padded) widths, copied verbatim: opaque, and only meaningful to the build and configuration that wrote it.
struct StateArgs {
  float* rec;                  // frame-0 (import) / frame-T (export) slot records [R][N][rec::W]
  float* temporal;             // [R][N][snh]
  float* prior;                // [R][N][psnh]
  float* last_id;              // [R]
  int* t_row;                  // [R] frame counter of each row at frame 0 of the pass
  float* fresh;                // import, training with a carried state: [R][N] 1 = the row starts fresh, 0 = imported; or NULL
  const float* blob_in;        // import: NULL = every row fresh
  float* blob_out;             // export
  const int* src;              // import: source row of each row, -1 (or out of [-1, R)) = fresh; NULL = identity
  int R, n_rec, n_tmp, n_pri, row_words;
  int t0;                      // import: counter of a fresh row; export: frames of the pass (added to the counter)
};
int sq_launch_state_import(const StateArgs& a, hipStream_t s);
int sq_launch_state_export(const StateArgs& a, hipStream_t s);

// SMC resampling of the carried state (sqair_set_smc): one workgroup per lane b, thread k = particle k of the lane (K <= 256).
struct SmcArgs {
  const float* lw;             // this pass's log_weights_per_timestep [T][R]
  const int* t_row;            // [R] frame counter of each row at frame 0 of the pass
  const float* uniforms;       // [B] or NULL: Philox keyed by (seed, b, counter of row b*K after the pass)
  float* log_w;                // [R] in/out
  float* log_z;                // [B] in/out
  float* log_evidence;         // [B] out
  float* ess;                  // [B] out
  float* u_out;                // [B] out or NULL
  int* resampled;              // [B] out
  int* src;                    // [R] out: source map of the next pass's k_state_import
  unsigned long long seed;
  float ess_frac;
  int T, B, K;
};
int sq_launch_smc_resample(const SmcArgs& a, hipStream_t s);

// Track history (sqair_set_history / sqair_history_trace).  The ring, 32-bit words:
//   header [SQ_HIST_HDR]: word 0 = passes pushed so far (advanced by k_history_push), word 1 = its workgroups' arrival count
//   trace scratch [L][R]: the ancestor rows of the last trace (k_history_walk -> k_history_gather / k_track_table)
//   L slots of `slot_words`: parent [R] | t0 [R] | where [T][R][N][4] | presence [T][R][N] | obj_id [T][R][N] |
//                            what [T][R][N][nw] (with the field) | log_w [T][R] (with the field)
constexpr int SQ_HIST_HDR = 64;
constexpr int SQ_HIST_PUSH_WORDS = 1024;   // words of a slot one workgroup of k_history_push copies
constexpr int SQ_HIST_MAX_TRACKS = 1024;
struct HistLayout {
  int L, T, R, N, nw, K;
  unsigned fields;
  long long o_where, o_pres, o_id, o_what, o_lw;   // offsets inside a slot (parent at 0, t0 at R); -1: field absent
  long long slot_words, scratch, slots, total;     // words; scratch / slots: offsets from the ring's base
};
struct HistPushArgs {
  unsigned* ring;
  HistLayout lay;
  const float *where, *presence, *obj_id, *what, *lw;   // the pass's outputs
  const int* src;       // the map the pass imported through, or NULL = identity
  int have_in;          // 0: no state_in, every row started fresh
  const int* t_row;     // [R]
};
int sq_launch_history_push(const HistPushArgs& a, hipStream_t s);
struct HistTraceArgs {
  unsigned* ring;
  HistLayout lay;
  const int* src_next;   // [R] or NULL
  int lag, M;
  float *where, *presence, *obj_id, *what, *log_w;
  int *valid, *frame_index, *ancestor_row, *unique_ancestors;
  int *track_id, *n_tracks;
  float *track_present, *track_where;
};
int sq_launch_history_trace(const HistTraceArgs& a, hipStream_t s);

// Generation modes (sqair_modules.py:157-170, :294-302).  Generation record of slot (r, k), 64 floats:
//   [0:4] where ~ prior, [4:54] what ~ prior, [54] presence ~ Bernoulli(prior logit), [55] the posterior path's own
//   propagation presence, [56] the posterior path's own discovery presence of step k
namespace gen {
#ifdef SQAIR_WIDE
constexpr int WHERE = 0, WHAT = 4, PRES = 132, ORIG_PRES = 133, ORIG_DPRES = 134, W = 144;
#else
constexpr int WHERE = 0, WHAT = 4, PRES = 54, ORIG_PRES = 55, ORIG_DPRES = 56, W = 64;
#endif
}
struct GenArgs {
  float* rec_p; float* rec_d; const float* rec_prev;   // records of this frame (overwritten when generating)
  const float* pstats; int ps_ld; const float* spre;   // prior statistics / where-prior conditioning of this frame
  const float* gen_noise;                              // frame slice of the second noise tensor [R][2][N][nzw]
  float* gen;                                          // generation records of this frame [R*N][64]
  const float* flat;
  int do_generate;
  SqairConfig cfg;
};
int sq_launch_generate_prop(const GenArgs& a, POff po, Dims d, hipStream_t s);
int sq_launch_generate_disc(const GenArgs& a, POff po, Dims d, hipStream_t s);

// Forecast (sqair_forecast): frame f of a rollout of the propagation prior from a carried state, discovery empty.  k_forecast_step
// samples every slot of a row from the prior statistics of this frame (the draws of k_generate_prop, same helpers), numbers the
// objects (compute_object_ids with no discovery) and compacts the N slots present-first into the next frame's records and prior
// states.  One wavefront per (row, slot).
struct ForecastArgs {
  const float* rec_prev;               // records of frame f - 1 [R][N][rec::W]
  const float* pstats; int ps_ld;      // raw prior linear output of this frame [(R*N)][ps_ld]
  const float* prior_p;                // the prior cell's new state of every slot [R][N][psnh]
  const float* noise;                  // noise of frame f [R][2][N][nzw] (slot s = 0 read)
  float* rec_next;                     // records of frame f [R][N][rec::W] (every word written)
  float* prior_next;                   // compacted prior states [R][N][psnh]
  int f;                               // frame index inside the outputs
  SqairForecastOutputs out;            // per-frame outputs (what, where, presence, presence_prob, presence_logit, obj_id)
  SqairConfig cfg;
};
int sq_launch_forecast_step(const ForecastArgs& a, Dims d, hipStream_t s);
// Missing-frame steps (sqair_set_observed): the frame of an unobserved (frame t, lane b) is the forecast's frame from the rows of
// t - 1 -- the same device function as k_forecast_step on section A's statistics of this frame -- with the temporal state of every
// slot held and carried through the same permutation.  k_coast_step runs right after the frame's k_compact and overwrites what
// that wrote for the rows of unobserved lanes; one wavefront per (row, slot), workgroups of observed lanes return at once.
struct CoastArgs {
  const int* observed;                 // [T][B] device, nonzero = the lane has a frame
  int t;                               // frame inside the pass (and inside the outputs)
  const float* rec_prev;               // records of frame t - 1 [R][N][rec::W]
  const float* pstats; int ps_ld;      // section A's prior statistics of this frame
  const float* prior_p;                // section A's new prior state of every slot [R][N][psnh]
  const float* temporal_prev;          // temporal state of frame t - 1 [R][N][snh]: held
  const float* noise;                  // noise of frame t [R][2][N][nzw] (slot s = 0 read)
  const float* last_id_prev; float* last_id_next;
  float* rec_next; float* prior_next; float* temporal_next;
  SqairOutputs out;
  SqairConfig cfg;
};
int sq_launch_coast_step(const CoastArgs& a, Dims d, hipStream_t s);
// k_coast_finish: one launch of the epilogue, one workgroup per (row, frame): for unobserved lanes every per-row and per-slot output
// the posterior path wrote becomes 0 (the log weight among them), the counts those of the coasted records.
struct CoastFinishArgs {
  const int* observed;                 // [T][B]
  const float* rec;                    // merged records of frames 0..T-1 [T][R][N][rec::W]
  int T;
  int train;                           // a masked carried training chunk: discrete_log_prob of a coasted row is its score term
  SqairOutputs out;
};
int sq_launch_coast_finish(const CoastFinishArgs& a, Dims d, hipStream_t s);
// The adjoint of the coasted frames of a masked carried chunk (sqair_glue.hip: k_coast_mask_grads, k_coast_step_bwd).
struct CoastMaskArgs {
  const int* observed;                 // [T][B]
  int T;
  float* g_lw; float* g_dl;            // [T][R] the objective's adjoint: zeroed for coasted (frame, row)s
  float* g_sc;                         // [T][R] out: the score term's coefficient of coasted (frame, row)s
};
int sq_launch_coast_mask_grads(const CoastMaskArgs& a, Dims d, hipStream_t s);
struct CoastBwdArgs {
  const int* observed;                 // [T][B]
  int t;
  const float* rec_prev;               // records of frame t - 1 [R][N][rec::W]
  const float* pstats; int ps_ld;      // section A's prior statistics of this frame
  const float* noise;                  // noise of frame t
  const float* g_sc;                   // [R] this frame's score coefficients
  const float* d_rec_next;             // gradient records of frame t [R][N][rec::W] (read at the slot's destination)
  const float* d_prior_next; const float* d_temporal_next;   // d prior_m / d temporal_m of frame t + 1
  float* d_rec_prev;                   // += gradient records of frame t - 1
  float* d_pstats;                     // += [R][N][ps_ld]
  float* d_prior_p;                    // =  [R][N][psnh]
  float* d_temporal_prev;              // += d temporal_m of frame t
  SqairConfig cfg;
};
int sq_launch_coast_step_bwd(const CoastBwdArgs& a, Dims d, hipStream_t s);
// Predictive summaries of a forecast of S rollouts per particle (rollout row q = r * S + s; S = 1: the plain forecast): one workgroup
// per (frame, lane b); w = softmax of the lane's K log weights (NULL: uniform), row q weighing w_{q / S} / S;
// mean_canvas[f][b] = sum_q w_q canvas[f][b*K*S + q], expected_count[f][b] = sum_q w_q (present slots of row q).  Every sum over q runs
// in index order.
struct ForecastSummaryArgs {
  const float* canvas;                 // [F][R*S][H*W]
  const float* rec;                    // records of frames 0..F-1 [F][R*S][N][rec::W]
  const float* log_w;                  // [R] or NULL
  float* mean_canvas;                  // [F][B][H*W] or NULL
  float* expected_count;               // [F][B] or NULL
  int F, B, K, S, N, P;
};
int sq_launch_forecast_summary(const ForecastSummaryArgs& a, hipStream_t s);

// The kernels of the per-lane answers (sqair_lane.hip) read the objects of a row through a view: slot j of row r at
// base + ((r * row_step) * N + j) * ld -- a pass's or a forecast's records (every ld = rec::W) or a caller's tensors (ld = 4, 1, 1).
struct LaneRows {
  const float* where; int where_ld;
  const float* presence; int pres_ld;
  const float* obj_id; int id_ld;
  int row_step;
};
// Lane estimates (sqair_set_estimate; include/sqair_hip.h states the semantics): k_lane_estimate, one workgroup per (lane b, frame t)
// -- times a third grid dimension over pixel chunks when mean_canvas is asked for, each recomputing the weights.  `rows`: row
// t * R + r is row r of frame t (row_step = 1); `what` at what + ((t * R + r) * N + j) * what_ld.
constexpr int SQ_EST_PIXELS = 1024;   // pixels of mean_canvas per workgroup of the third grid dimension
struct LaneEstArgs {
  LaneRows rows;
  const float* what; int what_ld;      // NULL unless est.what is set
  const float* canvas;                 // [T][R][H*W]; NULL unless est.mean_canvas is set
  const float* lw;                     // the pass's log_weights_per_timestep [T][R]
  SqairLaneEstimate est;               // iou_min, log_w and the outputs
  int T, B, K, N, nw, H, W;
};
int sq_launch_lane_estimate(const LaneEstArgs& a, hipStream_t s);
// Object layers (sqair_set_layers; include/sqair_hip.h states the semantics): k_lane_layers, one workgroup per (lane b, frame t,
// tile of SQ_LAYER_TILE consecutive pixels), each recomputing the lane's weights and association; a thread holds SQ_LAYER_PX pixels
// of every image in registers, so any frame size is a matter of the grid alone.  `rows` as LaneEstArgs' (obj_id is not read);
// glimpse (g) of slot m of row r of frame t at glimpse + (((t * R + r) * N + m) * G * G.
constexpr int SQ_LAYER_PX = 4, SQ_LAYER_TILE = 256 * SQ_LAYER_PX;
struct LaneLayerArgs {
  LaneRows rows;
  const float* glimpse;                // [T][R][N][G*G]
  const float* lw;                     // the pass's log_weights_per_timestep [T][R]
  const float* log_w;                  // the estimate's: [R] or NULL = zeros
  float iou_min;                       // the estimate's
  SqairLaneLayers lay;                 // cover_min and the outputs
  int T, B, K, N, G, H, W;
};
int sq_launch_lane_layers(const LaneLayerArgs& a, hipStream_t s);   // -2: the kernel's LDS (two glimpses) does not fit
// Stream scoring (sqair_set_score; include/sqair_hip.h states the semantics): k_lane_score, one workgroup per lane b looping over the
// pass's frames in order.  box / presence / obj_id [T][B][N] and map_count [T][B] are the estimate's outputs (or a test's buffers).
constexpr int SQ_SCORE_MAXG = 16;
struct LaneScoreArgs {
  const float* box;                    // [T][B][N][4]
  const float* presence;               // [T][B][N]
  const float* obj_id;                 // [T][B][N]
  const int32_t* map_count;            // [T][B]
  SqairLaneScore sc;                   // iou_min, G, the truth, the accumulators and the per-frame outputs
  int T, B, N;
  int match;                           // sqair_set_lane_match's score: 0 = keep + greedy (k_lane_score), 1 = keep + optimal (k_lane_score_opt)
};
int sq_launch_lane_score(const LaneScoreArgs& a, hipStream_t s);
// Lane identities (sqair_set_identity; include/sqair_hip.h states the semantics): k_lane_identity, one workgroup per lane b looping
// over the pass's frames in order, the track table in LDS across them.  box / presence / obj_id [T][B][N], what [T][B][N][nw] and
// best_row [T][B] are the estimate's outputs (or a test's buffers); what is read only when id.trk_what is set.
constexpr int SQ_IDENT_MAXM = 16;
struct LaneIdentArgs {
  const float* box;                    // [T][B][N][4]
  const float* presence;               // [T][B][N]
  const float* obj_id;                 // [T][B][N]
  const float* what;                   // [T][B][N][nw]; NULL unless id.trk_what is set
  const int32_t* best_row;             // [T][B]
  SqairLaneIdentity id;                // the scalars, the memory, the counters and the per-frame outputs
  int T, B, N, nw;
  int match;                           // sqair_set_lane_match's identity, step 2: 0 = k_lane_identity, 1 = k_lane_identity_opt
  int motion;                          // sqair_set_motion: 0 = the kernels above; 1 = k_lane_identity_motion / _motion_opt, which read mo
  SqairLaneMotion mo;                  // the filter's scalars, its state and the per-frame outputs; zeros while motion is 0
};
int sq_launch_lane_identity(const LaneIdentArgs& a, hipStream_t s);
// Trajectory scoring (sqair_lane_traj_score; include/sqair_hip.h states the semantics): k_lane_traj_score, grid (lane b, chunk of
// SQ_TRAJ_FRAMES frames): every workgroup recomputes its lane's link, then thread = frame, looping over the truth slots.
constexpr int SQ_TRAJ_FRAMES = 256;
struct LaneTrajScoreArgs {
  SqairLaneTraj tab;                   // the lane forecast's or the lane tracks' table (or a test's buffers)
  SqairTrajTruth tr;                   // G, the anchor, the truth of the table's frames, keep_id
  SqairTrajScore sc;                   // iou_min, the accumulators and the per-call outputs
  int F, B, N;
  int match;                           // sqair_set_lane_match's traj_link: 0 = k_lane_traj_score, 1 = k_lane_traj_score_opt
};
int sq_launch_lane_traj_score(const LaneTrajScoreArgs& a, hipStream_t s);
// IDF1 scoring (sqair_set_idf; include/sqair_hip.h states the semantics): k_lane_idf, one workgroup per lane b looping over the pass's
// frames in order with the lane's table in LDS across them.  box / presence / ids [T][B][N] and map_count [T][B] are the words
// k_lane_score was handed (or a test's buffers); of `sc` the truth, iou_min, G and truth_match are read.
constexpr int SQ_IDF_MAXP = 64;
struct LaneIdfArgs {
  const float* box;                    // [T][B][N][4]
  const float* presence;               // [T][B][N]
  const float* ids;                    // [T][B][N] 32-bit id words
  const int32_t* map_count;            // [T][B]
  SqairLaneScore sc;                   // read-only here
  SqairLaneIdf idf;                    // P, the table and totals
  int T, B, N;
};
int sq_launch_lane_idf(const LaneIdfArgs& a, hipStream_t s);
// The solve (sqair_lane_idf_solve): k_lane_idf_solve, one wavefront per lane b: the table to LDS, sq_assign_optimal_i32, the clip's
// figures; for the lanes of `close` the figures into totals and the table freed.
struct LaneIdfSolveArgs {
  SqairLaneIdf idf;
  const int32_t* close;                // [B] or NULL
  int64_t* open;                       // [B][SQAIR_IDF_TOTALS] or NULL
  int32_t* assign;                     // [B][G] or NULL
  int G, B;
};
int sq_launch_lane_idf_solve(const LaneIdfSolveArgs& a, hipStream_t s);
// HOTA scoring (sqair_set_hota; include/sqair_hip.h states the semantics): k_lane_hota, one workgroup per lane b looping over the pass's
// frames in order, one record of the lane's clip log per scored frame.  box / presence / ids [T][B][N] and map_count [T][B] are the
// words k_lane_score was handed (or a test's buffers); of `sc` the truth and G are read.
constexpr int SQ_HOTA_MAXP = 64;
constexpr int SQ_HOTA_MAXL = 4096;
constexpr int SQ_HOTA_BINS = SQAIR_HOTA_ALPHAS + 1;   // a matched pair's bin: the number of thresholds its q reaches, 0..19
struct LaneHotaArgs {
  const float* box;                    // [T][B][N][4]
  const float* presence;               // [T][B][N]
  const float* ids;                    // [T][B][N] 32-bit id words
  const int32_t* map_count;            // [T][B]
  SqairLaneScore sc;                   // read-only here
  SqairLaneHota hota;                  // P, L, the column table, the log and totals_c
  int T, B, N;
};
int sq_launch_lane_hota(const LaneHotaArgs& a, hipStream_t s);
// The solve (sqair_lane_hota_solve): k_lane_hota_solve, one workgroup of four wavefronts per lane b: pass 1 over the records in order,
// the alignment scores, pass 2 with a wavefront per record, the figures; for the lanes of `close` the figures into the totals and the
// lane freed.
struct LaneHotaSolveArgs {
  SqairLaneHota hota;
  const int32_t* close;                // [B] or NULL
  int64_t* open_i;                     // [B][19][4] or NULL
  double* open_f;                      // [B][19][3] or NULL
  int64_t* open_c;                     // [B][4] or NULL
  int32_t* match;                      // [B][L][G] or NULL
  int G, N, B;
};
int sq_launch_lane_hota_solve(const LaneHotaSolveArgs& a, hipStream_t s);
// The track log (sqair_set_tracklog; include/sqair_hip.h states the semantics): k_lane_tracklog, one workgroup per lane b over the
// pass's frames in order, one record of the lane's ring per frame.  lane_id / track_len [T][B][N] and best_row [T][B] are the
// identity's and the estimate's outputs, box [T][B][N][4] the estimate's (or a test's buffers).
constexpr int SQ_TRACKLOG_MAXL = SQAIR_TRACKLOG_MAX_FRAMES;
constexpr int SQ_TRACKLOG_MAXC = SQAIR_TRACKLOG_MAX_TRACKS;
struct LaneTrackLogArgs {
  const int32_t* lane_id;              // [T][B][N]
  const int32_t* track_len;            // [T][B][N]
  const int32_t* best_row;             // [T][B]
  const float* box;                    // [T][B][N][4]
  SqairLaneTrackLog log;               // L, count and the records
  int T, B, N;
};
int sq_launch_lane_tracklog(const LaneTrackLogArgs& a, hipStream_t s);
// The solve (sqair_lane_tracklog_smooth): k_lane_tracklog_smooth, one workgroup per lane b: the window, the columns, then one thread
// per (column, axis) filters forward and smooths backward.  `work`: [B][lag][C] int32, the slot of every (frame, column).
struct LaneTrackLogSmoothArgs {
  SqairLaneTrackLog log;
  SqairTrackLogOut out;
  int32_t* work;
  float q, r, v0_var;
  int lag, C, N, B;
};
int sq_launch_lane_tracklog_smooth(const LaneTrackLogSmoothArgs& a, hipStream_t s);
// Track log scoring (sqair_lane_tracklog_score; include/sqair_hip.h states the semantics): k_lane_tracklog_score, one workgroup of
// four wavefronts per lane b, wavefront v = view v of the solve's table, walking the window's frames in order.
struct LaneTrackLogScoreArgs {
  SqairLaneTrackLog log;               // L, count and log_valid are read
  SqairTrackLogOut tab;                // the solve's outputs, read-only here
  SqairTrackLogTruth tr;               // G and the truth of the window's frames
  SqairTrackLogScore sc;               // iou_min and the outputs
  int lag, C, B;
  int match;                           // 0 = sq_assign_keep_greedy, 1 = sq_assign_keep_optimal (a wave-uniform branch of the one kernel)
};
int sq_launch_lane_tracklog_score(const LaneTrackLogScoreArgs& a, hipStream_t s);
// Motion calibration (sqair_lane_tracklog_fit; include/sqair_hip.h states the semantics): k_lane_tracklog_fit, workgroup (b, iq) of
// 256 threads, one thread per (ir, column, axis) of a round of candidates, walking the window's frames in order.
struct LaneTrackLogFitArgs {
  SqairLaneTrackLog log;               // L and log_box are read
  SqairTrackLogOut tab;                // the solve's outputs, read-only here: frame_index and state are read
  const int32_t* work;                 // [B][lag][C], the solve's slots, read-only here
  SqairTrackLogFit fit;                // the grid by value, the scalars and the outputs
  int lag, C, N, B;
};
int sq_launch_lane_tracklog_fit(const LaneTrackLogFitArgs& a, hipStream_t s);
// Track log stitching (sqair_lane_tracklog_stitch; include/sqair_hip.h states the semantics): k_lane_tracklog_stitch, one workgroup
// of 256 threads per lane b: the fragments' spans, the C x C table of link weights in LDS, wave 0's assignment, the chains, then one
// thread per (stitched column, axis) walks the solve's filter and smoother over the joined slots.
struct LaneTrackLogStitchArgs {
  SqairLaneTrackLog log;               // L, count, log_valid and log_box are read
  SqairTrackLogOut tab;                // the solve's outputs, read-only here
  const int32_t* work;                 // [B][lag][C], the solve's slots, read-only here
  SqairTrackLogStitch st;              // gate, max_gap and the link outputs
  SqairTrackLogOut out;                // the stitched table
  int32_t* work_out;                   // [B][lag][C], the slots of the stitched columns
  float q, r, v0_var;
  int lag, C, N, B;
};
int sq_launch_lane_tracklog_stitch(const LaneTrackLogStitchArgs& a, hipStream_t s);

// Object forecasts (sqair_forecast_fan; include/sqair_hip.h states the semantics).  Fan-out: rollout row q = r * S + s.
// k_forecast_fan_src expands the source map, src_fan[q] = src[q / S] (NULL: q / S), an index outside [0, R) of the blob -> -1.
int sq_launch_forecast_fan_src(const int* src, int* src_fan, int R, int S, hipStream_t s);
// The lane forecast: k_forecast_lane_start, one workgroup per lane (weights, best start row, its objects, the K x N association and
// the followed ids, left in `scratch`), then k_forecast_lane_frame, one workgroup per (lane, frame), thread = rollout.  Start row r
// is row r of the view `start` -- frame 0 of the forecast's records (row_step = S) or the caller's tensors (row_step = 1); slot j of
// (frame f, rollout row q) at base + (((f * R * S) + q) * N + j) * ld.
inline int64_t sq_al64(int64_t x) { return (x + 63) / 64 * 64; }
struct ForecastLaneScratch { float* w; unsigned* fid; int* fm; int* bp; };   // [R], [R][N], [R][N], [B][N]
inline int64_t sq_forecast_lane_scratch_words(int64_t B, int64_t K, int64_t N) { return sq_al64(B * K) + 2 * sq_al64(B * K * N) + sq_al64(B * N); }
inline ForecastLaneScratch sq_forecast_lane_scratch(float* base, int64_t B, int64_t K, int64_t N) {
  ForecastLaneScratch x;
  x.w = base; base += sq_al64(B * K);
  x.fid = (unsigned*)base; base += sq_al64(B * K * N);
  x.fm = (int*)base; base += sq_al64(B * K * N);
  x.bp = (int*)base;
  return x;
}
struct ForecastLaneArgs {
  LaneRows start;
  const float* where; int where_ld;
  const float* presence; int pres_ld;
  const float* obj_id; int id_ld;
  const float* log_w;                  // [R] or NULL
  ForecastLaneScratch x;
  SqairForecastLane lane;              // iou_min and the outputs
  int F, B, K, S, N, H, W;
};
int sq_launch_forecast_lane(const ForecastLaneArgs& a, hipStream_t s);
// Lane tracks (sqair_history_trace_lane; include/sqair_hip.h states the semantics): the lane forecast's two kernel bodies run backwards
// in time over the K traced paths of a lane.  `f` is the forecast's block with S = 1: where / presence / obj_id = the traced rows
// [F][R][N] (ld = 4, 1, 1), `start` = the view of their frame F - 1, `lane` = the outputs the two answers share (start_* NULL), the
// same scratch.  What the tracks add: the rows' `valid` mask and the two outputs the forecast has no counterpart of.
struct TrackLaneArgs {
  ForecastLaneArgs f;
  const int* valid;                    // [F][R]
  int* first_frame;                    // [B][N] or NULL
  float* valid_mass;                   // [F][B] or NULL
};
int sq_launch_track_lane(const TrackLaneArgs& a, hipStream_t s);

struct CompactArgs {
  const float* rec_p; const float* rec_d; const float* rec_prev;
  const float* temporal_p; const float* prior_p;
  const float* last_id_prev; float* last_id_next;
  float* rec_next; float* temporal_next; float* prior_next;
  const float* flat;
  int t;
  SqairOutputs out;
  int* src_out;            // optional (training): source slot (0..2N-1) of every surviving slot [R,N]
};
int sq_launch_compact(const CompactArgs& a, POff po, Dims d, hipStream_t s);

struct InsertArgs {
  const float* glimpse;    // [R,N,G*G]
  const float* rec;        // merged records of this frame [R,N,rec_ld] (where at +0, presence at +54) or
  int rec_ld;              // plain mode: where [R,N,4] / presence [R,N] given separately
  const float* where_plain; const float* pres_plain;
  const float* img;        // [B,H,W]
  const float* mean_img;   // [H,W]
  float* canvas;           // optional [R,H,W]
  float* data_ll;          // [R]
  const float* qz; const float* pz;  // optional frame scalars -> log weight outputs
  int t;                   // first frame in the output tensors
  int n_frames;            // frames covered by the launch (0/1 = single)
  SqairOutputs out;        // only the scalar log-weight outputs are used (may be all NULL)
  float std_fg, std_bg;
};
int sq_launch_insert_loglik(const InsertArgs& a, Dims d, hipStream_t s);
// The same kernels instantiated without an observation (forecast): canvas only -- img, data_ll, qz / pz and the scalar outputs are
// not read or written.  a.canvas must be set.
int sq_launch_insert_canvas(const InsertArgs& a, Dims d, hipStream_t s);

int sq_launch_elbo(const float* log_w_t, const float* disc_lp_t, int T, int B, int K, float* log_weights,
                   float* elbo_per_ex, float* iw, float* signal, float* scalars, const float* const* means_in,
                   int n_means, float* means_out, hipStream_t s, int reinforce = 0);
