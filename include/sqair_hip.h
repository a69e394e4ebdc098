/*
 * sqair_hip.h — C-ABI of the MI355X-native SQAIR Discover/Propagate hot path (libsqair_hip.so).
 *
 * The reference (akosiorek/sqair) has no native/FFI layer: its operator API for this path is the
 * Python factory  load(img, coords, num, mean_img, debug) -> Model
 *   (reference: sqair/configs/mlp_mnist_model.py:74-150, called through
 *    sqair/experiment_tools.py:147-157 from sqair/scripts/experiment.py:118 and scripts/eval.py:138)
 * and the Model object it returns (reference: sqair/model.py:33-214).  This header is the boundary a
 * maintainer would bind from that Python side (ctypes stub in INTEGRATION.md); sqair_amd/ mirrors
 * load()/Model on top of it.
 *
 * Conventions
 *   - plain C symbols, no C++/torch types; every tensor is caller-owned DEVICE memory, contiguous
 *     row-major float32 (HBM-resident torch tensors' data_ptr() in practice);
 *   - the library allocates no device memory: parameters are re-laid-out into a caller-provided
 *     "packed" buffer, all intermediates live in a caller-provided workspace;
 *   - every launch function takes a hipStream_t (passed as void*) and is asynchronous on it;
 *   - return value 0 = ok, negative = error (message via sqair_last_error); one handle per
 *     (device, stream), not thread-safe across threads sharing a handle.
 *
 * Row convention: B' = B*K rows, particle-contiguous (b' = b*K + k), the layout
 * index.tile_input_for_iwae produces (reference: sqair/index.py:106-129) — the tiled observation is
 * never materialised, kernels index obs[t, b'/K].
 */
#ifndef SQAIR_HIP_H
#define SQAIR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQAIR_ABI_VERSION 2   /* 2: sqair_build_id / sqair_build_flags added, sqair_profile_* removed */

/* Hyper-parameters of the path.  Field names follow the reference flags
 * (reference: sqair/common_model_flags.py:32-56, sqair/configs/mlp_mnist_model.py:42-52). */
typedef struct SqairConfig {
  int32_t img_h, img_w;          /* H, W of a (grayscale) frame                                  */
  int32_t glimpse_size;          /* G, flag glimpse_size                                         */
  int32_t n_steps_per_image;     /* N object slots, flag n_steps_per_image                       */
  int32_t n_what;                /* flag n_what                                                  */
  int32_t n_hidden;              /* 32 * n_units (get_params, common_model_flags.py:59-71)       */
  int32_t k_particles;           /* K, flag k_particles                                          */
  int32_t prop_prior_type;       /* 0 = rnn, 1 = rw, 2 = guided (propagate.py:36-40)             */
  int32_t disc_prior_type;       /* 0 = cat, 1 = geom (sqair_modules.py:204-224)                 */
  int32_t masked_glimpse;        /* flag masked_glimpse                                          */
  int32_t rec_where_prior;       /* flag rec_where_prior                                         */
  float prop_prior_step_bias;    /* flag prop_prior_step_bias                                    */
  float step_success_prob;       /* flag step_success_prob (geom prior only)                     */
  float output_std;              /* effective p(x|z) std: fl32(fl32(sqrt(flag))^2), modules.py:419-422 */
  float background_std;          /* same for background pixels (bg_std=None -> output_std)       */
  float where_prior_mean[4];     /* scale_prior x2, 0, 0 (non-recurrent where prior only)        */
  int32_t sample_from_prior;     /* flag sample_from_prior (mlp_mnist_model.py:51): needs sqair_set_generation_noise */
  int32_t generate_after;        /* SequentialAIR(generate_after=..) (seq.py:46, :198-200); <= 0: never generate     */
  int32_t time_cell;             /* flag time_transition: 0 = GRU (shipped), 1 = LSTM, 2 = VanillaRNN (common_model_flags.py:49) */
  int32_t prior_cell;            /* flag prior_transition: 0 = GRU (shipped), 1 = LSTM, 2 = VanillaRNN (mlp_mnist_model.py:125)  */
  int32_t rnn_cell;              /* flag transition (slot RNN of both cores): 0 = VanillaRNN (shipped), 1 = LSTM, 2 = GRU */
} SqairConfig;

typedef struct SqairHandle SqairHandle;

/* ---- lifetime / introspection (host only: usable without a GPU) -------------------------------- */
int sqair_abi_version(void);
/* Identity of the loaded binary: 16 hex digits = sha256 over the sources it was compiled from (sqair_amd/csrc/ + this header +
 * compiler flags; sqair_amd/csrc/build.py computes the same hash over the files on disk), and the build variant
 * ("product" | "timeline" | "knobs").  Measurements are quoted next to this id, and the Python binding refuses a binary whose
 * id is not the id of the sources beside it. */
const char* sqair_build_id(void);
const char* sqair_build_flags(void);
/* Returns -1 for a configuration outside this BUILD's limits.  libsqair_hip.so (the product) is laid out for the shipped model family:
 * n_what <= 50, n_steps_per_image <= 8, n_hidden <= 256; libsqair_hip_wide.so -- the same sources compiled with -DSQAIR_WIDE, the
 * same C-ABI, slower per-row kernels -- takes n_what <= 128, n_steps_per_image <= 16 (15, 16 only while the log-probability
 * adjoint's LDS staging fits: not with its 416-float slot record), n_hidden <= 512.  Both: n_hidden = 32 * n_units any multiple
 * of 16 (the kernels run on the next of 128 / 256 / 512 with inert padding units; parameters, gradients and final states cross
 * this ABI in the reference's shapes), k_particles <= 256, any H x W for inference; TRAINING (sqair_forward_train /
 * sqair_backward) takes frames up to 38 400 pixels (150 KB: the crop adjoint stages the frame in LDS) and says so at entry.
 * The reference's flags take any value
 * (sqair/common_model_flags.py:32-56, sqair/configs/mlp_mnist_model.py:42-52); a host picks the library by the flags
 * (sqair_amd/_capi.py: lib_path_for). */
int sqair_create(const SqairConfig* cfg, SqairHandle** out);
int sqair_destroy(SqairHandle* h);
const char* sqair_last_error(const SqairHandle* h);

/* Flat parameter buffer = the reference's trainable variables in the order of SURVEY.md Appendix C
 * (reference listing: notebooks/play.ipynb:239-362), each row-major fp32, no padding.
 * sqair_param_entry enumerates (name, offset, numel) so the Python side can cross-check its spec. */
int64_t sqair_param_count(const SqairHandle* h);
int sqair_param_entries(const SqairHandle* h);
int sqair_param_entry(const SqairHandle* h, int i, const char** name, int64_t* offset, int64_t* numel);

/* Sizes (bytes) of the caller-provided buffers. */
int64_t sqair_packed_bytes(const SqairHandle* h);
int64_t sqair_workspace_bytes(const SqairHandle* h, int T, int B);
int sqair_noise_width(const SqairHandle* h); /* 4 + n_what + 1 */
int sqair_get_config(const SqairHandle* h, SqairConfig* out);

/* ---- parameters ------------------------------------------------------------------------------- */
/* Re-lays the flat parameters out for the MFMA kernels (16x16x4-fp32 fragment order, K padded per
 * input segment, loop-invariant sub-matrices grouped) into `packed`.  Call after every parameter
 * update.  Replaces variable creation inside load() (mlp_mnist_model.py:99-148). */
int sqair_pack_params(SqairHandle* h, const float* flat_params, void* packed, void* stream);

/* ---- the forward pass --------------------------------------------------------------------------
 * Per-frame outputs, every pointer optional (NULL = not written); shapes are [T, B', ...] exactly
 * as the TensorArrays of SequentialAIR (reference: sqair/seq.py:121-177).  */
typedef struct SqairOutputs {
  float* what;                       /* [T,B',N,n_what] */
  float* what_loc;                   /* [T,B',N,n_what] */
  float* what_scale;                 /* [T,B',N,n_what] */
  float* where;                      /* [T,B',N,4] */
  float* where_loc;                  /* [T,B',N,4] */
  float* where_scale;                /* [T,B',N,4] */
  float* presence_prob;              /* [T,B',N] */
  float* presence;                   /* [T,B',N] */
  float* presence_logit;             /* [T,B',N] */
  float* obj_id;                     /* [T,B',N] */
  float* step_log_prob;              /* [T,B'] */
  float* canvas;                     /* [T,B',H,W] */
  float* glimpse;                    /* [T,B',N,G,G] */
  float* disc_what_log_prob;         /* [T,B',N] */
  float* disc_where_log_prob;        /* [T,B',N] */
  float* disc_what_prior_log_prob;   /* [T,B',N] */
  float* disc_where_prior_log_prob;  /* [T,B',N] */
  float* disc_log_prob;              /* [T,B'] */
  float* disc_prior_log_prob;        /* [T,B'] */
  float* disc_prob;                  /* [T,B',N+1] */
  float* prop_what_log_prob;         /* [T,B',N] */
  float* prop_where_log_prob;        /* [T,B',N] */
  float* prop_what_prior_log_prob;   /* [T,B',N] */
  float* prop_where_prior_log_prob;  /* [T,B',N] */
  float* prop_log_prob;              /* [T,B'] */
  float* prop_prior_log_prob;        /* [T,B'] */
  float* prop_prob;                  /* [T,B',N] */
  float* discrete_log_prob;          /* [T,B'] */
  float* num_prop_steps_per_sample;  /* [T,B'] */
  float* num_disc_steps_per_sample;  /* [T,B'] */
  float* num_steps_per_sample;       /* [T,B'] */
  float* prop_pres;                  /* [T,B',N] */
  float* disc_pres;                  /* [T,B',N] */
  float* data_ll_per_sample;         /* [T,B'] */
  float* kl_per_sample;              /* [T,B'] */
  float* log_q_z_given_x_per_sample; /* [T,B'] */
  float* log_p_z_per_sample;         /* [T,B'] */
  float* log_weights_per_timestep;   /* [T,B']  (required by sqair_elbo) */
  /* not reference outputs: final recurrent state, for state-level parity checks */
  float* final_temporal_state;       /* [B',N,n_hidden] */
  float* final_prior_state;          /* [B',N,n_hidden] */
  float* final_last_used_id;         /* [B'] */
} SqairOutputs;

/* Unrolls the model over T frames: replaces SequentialAIR.__call__ on the tiled observation
 * (reference: sqair/seq.py:69-84 -> _loop_body :179-269 -> SQAIRTimestep sqair_modules.py:446-582 ->
 * Propagate/Discover -> PropagationCore/DiscoveryCore sqair/core.py:164-359 -> AIRDecoder
 * sqair/modules.py:435-467 -> _compute_log_weights seq.py:271-276).
 *   obs    [T,B,H,W] in [0,1]
 *   noise  [T,B',2,N,noise_width]: s=0 propagation slot k, s=1 discovery step k; entries 0:4 eps of
 *          `where`, 4:4+n_what eps of `what`, last = uniform u of the presence Bernoulli
 *   t_offset: index of obs[0] in the full sequence (the categorical step prior is time dependent,
 *          sqair_modules.py:212-215); 0 for a whole sequence. */
int sqair_forward(SqairHandle* h, const float* flat_params, const void* packed, const float* obs,
                  const float* noise, int T, int B, int t_offset, const SqairOutputs* out,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* Training-mode forward pass: same launch sequence and results, but every intermediate the backward pass needs
 * (per-frame and per-slot activations, GRU gates, compaction permutation) is kept in the larger workspace of
 * sqair_train_workspace_bytes; sqair_backward consumes it. */
int64_t sqair_train_workspace_bytes(const SqairHandle* h, int T, int B);
int sqair_forward_train(SqairHandle* h, const float* flat_params, const void* packed, const float* obs,
                        const float* noise, int T, int B, int t_offset, const SqairOutputs* out,
                        void* workspace, int64_t workspace_bytes, void* stream);

/* Same launch sequence recorded once into a HIP graph and replayed (the T x 2N sequential steps
 * are launch-latency bound).  Pointers are frozen at capture time: the caller keeps the same
 * buffers and refreshes their contents before each sqair_graph_launch. */
int sqair_graph_capture(SqairHandle* h, const float* flat_params, const void* packed, const float* obs,
                        const float* noise, int T, int B, int t_offset, const SqairOutputs* out,
                        void* workspace, int64_t workspace_bytes, void* stream);
int sqair_graph_launch(SqairHandle* h, void* stream);
int sqair_graph_nodes(const SqairHandle* h); /* kernel nodes in the captured graph */

/* ---- carried model state (streaming inference) ----------------------------------------------------
 * A pass normally starts every particle row from the trainable initial state.  With a state set, the following sqair_forward /
 * sqair_graph_capture calls (and sqair_forward calls between sqair_capture_begin / _end) of this handle instead start each row
 * from a state blob and write the state after their last frame into another (or the same) blob, so that a sequence can be fed
 * in chunks of any length -- down to one frame per call -- with the same results as one pass over the whole sequence.
 * A blob row holds everything frame t + 1 reads of frame t: the N slot records (what / where / presence / logit / id ...), the
 * temporal and propagation-prior cell states, the last used object id, and the row's frame counter (the index the
 * time-dependent step prior sees; it replaces t_offset).  The blob is OPAQUE: device memory of sqair_state_bytes(h, B) bytes,
 * only meaningful to a handle of the same build (product / wide), configuration and B.
 *   state_in   NULL: every row starts fresh at t_offset (the state after the pass is still exported);
 *   state_out  NULL: nothing is exported; may equal state_in (import happens in the prologue, export at the end of the pass,
 *              in stream order: one captured graph can then be replayed frame after frame);
 *   src_rows   optional device int32[B*K]: row r is imported from blob row src_rows[r]; -1 (or any index outside [-1, B*K))
 *              starts row r fresh (counter 0).  Resets lanes, resamples particles (src[b*K + k] = b*K + k'), recomposes a
 *              batch.  NULL = identity.  Needs state_in.
 * All three NULL switches the state off.  Pointers are remembered by the handle and frozen into captured graphs.  Refused
 * (return -1, text in sqair_last_error, before any HIP call): sqair_forward_train / sqair_backward while a state is set (training
 * with a carried state has its own calls, sqair_forward_train_carry / sqair_backward_carry, below), a
 * configuration with sample_from_prior, t_offset != 0 with state_in set, a pass whose B is not the B given here, and
 * state_bytes < sqair_state_bytes(h, B). */
int64_t sqair_state_bytes(const SqairHandle* h, int B);
int sqair_set_state(SqairHandle* h, const void* state_in, void* state_out, const int32_t* src_rows, int64_t state_bytes, int B);

/* ---- SMC resampling of a carried state (adaptive particle filter) --------------------------------------------------
 * A pass's per-frame log weight (log_weights_per_timestep) is the incremental importance weight of a particle filter whose
 * proposal is the inference network.  With SMC set, every following pass with a carried state ends with one more kernel (after
 * the state export) that, per lane b (sequence), turns the lane's weights into the source map of the NEXT pass, on the device:
 *   a_k = log_w[b*K + k] + sum over this pass's frames of log_weights_per_timestep   (frame order, fp32)
 *   m = max_k a_k, e_k = exp(a_k - m), S = sum e_k, ESS = S^2 / sum e_k^2        (fixed order: same bits on every replay)
 *   log_evidence[b] = log_z[b] + m + log(S / K)    (SMC estimate of log p(x_1..t)),  ess[b] = ESS   (both before resampling)
 *   resample iff ess_frac == 1 or ESS < ess_frac * K:
 *     systematic, one u per lane (uniforms[b], or Philox keyed by (seed, b, frame counter of row b*K after the pass)):
 *     src_rows[b*K + j] = b*K + (smallest k with c_k > (j + u) * S / K; if fp32 rounding leaves none, the first k with
 *     c_k = S: the last particle of positive weight, never a zero-weight one), c = inclusive prefix sum of e;
 *     log_z[b] += m + log(S / K), log_w of the lane = 0, resampled[b] = 1
 *   otherwise: src_rows of the lane = identity, log_w[b*K + k] = a_k, resampled[b] = 0.
 *   A lane whose ESS is not finite (a NaN or +inf a_k, or every a_k at -inf) never resamples, whatever ess_frac: identity map,
 *   a_k carried in log_w unchanged, log_z kept, resampled[b] = 0; its ess and log_evidence show the non-finite value.
 * The next pass's state import gathers the rows through src_rows (records, cell states, ids, counters): the path a caller's
 * own source map takes.  Resampling happens at pass boundaries only: one-frame passes give per-frame SMC.
 * u_out[b] receives the lane's uniform of the pass whether or not the lane resampled.
 * Pointers are remembered by the handle and frozen into captured graphs, as the state's are.  A sqair_set_state call that
 * switches the state off (all NULL), drops state_in, or changes the source map or B switches SMC off too.  NULL smc: off.  Refused (return -1, text in sqair_last_error, before
 * any HIP call): no state set, a state without state_in or without a source map, src_rows other than the state's source map,
 * ess_frac NaN or outside [0, 1], a NULL log_w / log_z / log_evidence / ess / resampled, a B other than the state's; and at
 * pass time, a pass with SMC on whose out->log_weights_per_timestep is NULL. */
typedef struct {
  float ess_frac;            /* resample iff ess_frac == 1 or ESS < ess_frac * K; 0 = never */
  uint64_t seed;             /* Philox key when uniforms == NULL */
  const float* uniforms;     /* [B] or NULL */
  float* log_w;              /* [B*K] in/out: log weights accumulated since the lane's last resampling */
  float* log_z;              /* [B]   in/out: log evidence banked at resamplings */
  float* log_evidence;       /* [B] out */
  float* ess;                /* [B] out, before resampling */
  float* u_out;              /* [B] out or NULL */
  int32_t* resampled;        /* [B] out */
  int32_t* src_rows;         /* must be the source map given to sqair_set_state; written for the next pass */
} SqairSmc;
int sqair_set_smc(SqairHandle* h, const SqairSmc* smc, int B);   /* NULL smc: off */
/* Kernel-level check of the resampler (tests): the kernel above on caller buffers, no state and no pass.  lw [T][B*K] stands for
 * the pass's log_weights_per_timestep, t_row [B*K] for the rows' frame counters at frame 0 of the pass (read only for Philox,
 * when smc->uniforms is NULL; may then be NULL otherwise), smc->src_rows [B*K] receives the map.  1 <= K <= 256.  Refused
 * (return -1, before any HIP call): NULL lw / smc, T, B or K out of range, ess_frac NaN or outside [0, 1], a NULL log_w / log_z /
 * log_evidence / ess / resampled / src_rows, or no uniforms and no t_row. */
int sqair_smc_resample_test(SqairHandle* h, const float* lw, int T, int B, int K, const int32_t* t_row, const SqairSmc* smc,
                            void* stream);

/* ---- track history: the last L passes kept on the device, traced into fixed-lag smoothed trajectories -------------------------
 * With a history set, every following inference pass with a carried state ends with one more kernel, k_history_push, after the
 * state export and BEFORE the SMC resampler (which overwrites the source map the push records).  It writes slot (passes pushed
 * so far) mod L of a ring, an OPAQUE device blob of sqair_history_bytes(h, L, T, B, fields) bytes that the caller ZERO-FILLS before
 * registering it (zeroing it again forgets the history).  A slot holds, for one pass of T frames:
 *   the chosen per-frame outputs [T, B*K, N, .] in their own widths (n_what, not the record's padded width), 32-bit words copied
 *     as they are out of the pass's SqairOutputs buffers (the pass must bind them: a NULL one is refused at pass time);
 *   parent[B*K]  the source map the pass imported through, as k_state_import read it: -1 = the row started fresh (also: no
 *     state_in, an index outside [0, B*K)), identity without a map;
 *   t0[B*K]      the row's frame counter at frame 0 of the pass (the index the time-dependent step prior saw).
 * The number of passes pushed lives in the ring's header ON THE DEVICE; the kernel reads and advances it, so one captured graph
 * serves every pass, the wrap-around included.  All passes pushed into one ring have the same T (a pass with another T is refused).
 * A pass with history on has exactly one graph node more; with history off nothing is launched.
 * `fields`: a bit set; where, presence and obj_id are mandatory.
 * Refused (return -1, text in sqair_last_error, before any HIP call): no state set, L < 1, fields without the mandatory three or
 * with unknown bits, ring_bytes < sqair_history_bytes(h, L, 1, B of the state, fields); at pass time: a B other than the
 * state's, ring_bytes < sqair_history_bytes for the pass's T, a T other than the ring's earlier passes', a NULL output among the
 * fields.  NULL ring: off.  sqair_set_state switching the state off switches history off too.  Training passes
 * (sqair_forward_train*, sqair_forward_train_carry) never push: a history for training on streams is out of scope.
 * The ring's T is fixed by the first pass that none of the pass-time refusals -- the history's own or another registration's, the
 * estimate's for instance -- turns away: a refused pass leaves the handle, the ring's T included, as it was. */
#define SQAIR_HIST_WHERE    1u
#define SQAIR_HIST_PRESENCE 2u
#define SQAIR_HIST_OBJ_ID   4u
#define SQAIR_HIST_WHAT     8u
#define SQAIR_HIST_LOG_W    16u   /* log_weights_per_timestep */
#define SQAIR_HIST_MANDATORY 7u
#define SQAIR_HIST_ALL       31u
int64_t sqair_history_bytes(const SqairHandle* h, int L, int T, int B, uint32_t fields);   /* -1: bad arguments */
int sqair_set_history(SqairHandle* h, void* ring, int64_t ring_bytes, int L, uint32_t fields);
/* Traces the ancestral path of every particle row back over the last `lag` passes of `ring` (the ring registered with
 * sqair_set_history; 1 <= lag <= L): the trajectories of the surviving particles, i.e. the fixed-lag smoothing distribution of
 * the filter.  Passes never pushed, or already overwritten, count as absent.
 * Start rows:  src_next == NULL: the rows of the LAST pass's outputs, a = r;
 *              src_next [B*K] : the rows the NEXT pass would start from, a = src_next[r] (the forecast's convention; after an
 *                               SMC resampling the equally weighted surviving set); -1 (or out of range) gives an empty path.
 * The walk, from the newest pass i = lag - 1 to the oldest i = 0:  ancestor_row[i, r] = a;  a = parent_i[a].  A fresh row (-1)
 * ends the path: every older frame of r is invalid.
 * Outputs, every pointer optional, frames ordered oldest -> newest, frame f = i * T + t of F = lag * T:
 *   where / presence / obj_id / what / log_w: the stored 32-bit words of the ancestor's row, zero where invalid (what / log_w
 *     only when the ring holds the field);  valid = 1 / 0;  frame_index = t0 + t, -1 where invalid;
 *   unique_ancestors[i, b]: the number of distinct ancestor rows among lane b's K paths at pass i (path degeneracy: how far
 *     back the smoothing still has more than one hypothesis).
 * Track table (any of the track_* pointers set; max_tracks = M >= 1): slots are not tracks, compaction moves an object between
 * them.  Per traced row, the ids present (presence == 1) in at least one valid frame of its path, ascending, the first M of them:
 *   track_id [R, M] (-1 padded), n_tracks [R] the true distinct count (above M: the table was truncated),
 *   track_present [F, R, M] 1 / 0 and track_where [F, R, M, 4], zero where the id is absent in that frame.
 * Everything is a copy or an integer count: the same bits on every replay.  Writes `out` and the ring's own trace scratch only
 * (nothing a pass reads), so it may interleave with passes; capturable (no host sync, no allocation).  One trace at a time per ring.
 * Refused (return -1, text in sqair_last_error, before any HIP call): no history set or a ring other than the registered one,
 * lag < 1 or > L, a NULL out, out->T < 1 or other than the T of the passes pushed, what / log_w asked of a ring without the
 * field, a track pointer with max_tracks outside [1, 1024]. */
typedef struct SqairTraceOutputs {
  int32_t T;                 /* frames per pass the buffers are sized for (F = lag * T) */
  int32_t max_tracks;        /* M of the track table; read only when a track_* pointer is set */
  float* where;              /* [F,B',N,4] */
  float* presence;           /* [F,B',N] */
  float* obj_id;             /* [F,B',N] */
  float* what;               /* [F,B',N,n_what] */
  float* log_w;              /* [F,B'] */
  int32_t* valid;            /* [F,B'] */
  int32_t* frame_index;      /* [F,B'] */
  int32_t* ancestor_row;     /* [lag,B'] */
  int32_t* unique_ancestors; /* [lag,B] */
  int32_t* track_id;         /* [B',M] */
  int32_t* n_tracks;         /* [B'] */
  float* track_present;      /* [F,B',M] */
  float* track_where;        /* [F,B',M,4] */
} SqairTraceOutputs;
int sqair_history_trace(SqairHandle* h, void* ring, const int32_t* src_next, int lag, const SqairTraceOutputs* out,
                        void* stream);
/* ---- lane tracks: one smoothed trajectory per object of a lane ---------------------------------------------------------------
 * sqair_history_trace answers per particle row: K ancestral paths per lane.  sqair_history_trace_lane runs the same trace and then
 * turns the K traced paths of a lane into one answer per object of the lane -- where it was, frame by frame, with the weight of the
 * particles that agree and their spread: the backward-looking twin of the lane forecast (SqairForecastLane), by the same device
 * functions, so that between the same two steps both list the same objects in the same order and past and future join into one
 * trajectory per object.  R = B*K, F = lag*T, frames oldest -> newest.  Row r of traced frame f is the trace's gathered row: its
 * ancestor's stored words (zero where invalid) plus valid[f, r].  log_w [R] (NULL: uniform) weighs the traced rows: with src_next
 * the weights of the rows the next pass would start from.  Per lane b:
 * 1. Weights and best row: sqair_forecast_fan's point 1 on log_w, the same device helpers: weights[b,k] = w_k, best_row[b] = b*K +
 *    the first k of maximal log weight.
 * 2. The lane's objects are the slots j of the best row's NEWEST traced frame (f = F-1): presence, obj_id [B,N] copied words,
 *    box0 [B,N,4] = (y, x, h, w) in pixels; all zero where the slot is absent or where that frame of the best row is invalid.
 * 3. Association, ONCE, on frame F-1, by sqair_set_estimate's point 5: per object j and particle k, m* = the first present slot of
 *    k's row of maximal IoU with box0[j]; k is associated with j when that IoU >= iou_min, and the obj_id word of slot m* is the id
 *    FOLLOWED back along k's path.  A particle whose frame F-1 is invalid is associated with nothing.
 *    support[b,j] = sum_k w_k [k associated].
 * 4. Per frame f and object j, over the particles k that are associated, valid at f, and hold a present slot of their row at f
 *    whose obj_id word equals the followed id (an exact compare; the first such slot):
 *      alive[f,b,j]    = sum w_k             (unnormalised; alive[F-1] is support bit for bit)
 *      box_mean[f,b,j] = sum w_k box_k / alive
 *      box_std[f,b,j]  = sqrt(sum w_k (box_k - box_mean)^2 / alive)      (two passes in fp32, as the forecast's)
 *    Where alive is 0 (an object born inside the window, at older frames) the box statistics are NaN.  An absent object gives zeros.
 * 5. count_prob[f,b,c] = sum_k w_k [k valid at f and holds c present slots], c = 0..N;  valid_mass[f,b] = sum_k w_k [k valid at f].
 *    Both are left UNNORMALISED: count_prob[f,b,:] sums to valid_mass[f,b], not to 1 -- the mass of the paths that reach back to f.
 * 6. first_frame[b,j] (int32): the oldest f from which the best row's own path holds the id word obj_id[b,j] present in every
 *    frame up to F-1; -1 for an absent object.
 * 7. Every sum over particles is ONE thread's loop over k in index order: no float atomics, the same bits eager or replayed.
 *    Non-finite lanes follow sqair_forecast_fan's point 7: NaN weights, support, alive, box_mean, box_std, count_prob and
 *    valid_mass, best_row = -1 and no objects (presence, obj_id, box0 zero, first_frame -1).
 * 8. Writes only `out`, `lane`, the scratch (sqair_trace_lane_scratch_bytes(h, B, K) bytes of device memory) and the ring's trace
 *    scratch: capturable, and it interleaves with passes as sqair_history_trace does.  Two launches on top of the trace's.
 * Every pointer of SqairTraceLane is optional except best_row.
 * Refused (return -1, text in sqair_last_error, before any HIP call): everything sqair_history_trace refuses; a NULL lane or
 * best_row; iou_min NaN or outside (0, 1]; K > 256; lag * T > 65535; a NULL scratch or scratch_bytes too small; a NULL out->where,
 * out->presence, out->obj_id or out->valid (the lane kernels read the gathered rows).
 * Out of scope: objects that left the scene before frame F-1 are not part of the answer -- the per-row track table (track_id ...)
 * serves them; anchoring departed objects at their last present frame is a later step. */
typedef struct SqairTraceLane {
  float iou_min;             /* in (0, 1] */
  int32_t* best_row;         /* [B] required */
  float* weights;            /* [B,K] */
  float* obj_id;             /* [B,N] */
  float* presence;           /* [B,N] */
  float* box0;               /* [B,N,4] (y, x, h, w) in pixels, at frame F-1 */
  float* support;            /* [B,N] */
  int32_t* first_frame;      /* [B,N] */
  float* alive;              /* [F,B,N] */
  float* box_mean;           /* [F,B,N,4] */
  float* box_std;            /* [F,B,N,4] */
  float* count_prob;         /* [F,B,N+1] unnormalised */
  float* valid_mass;         /* [F,B] */
} SqairTraceLane;
int64_t sqair_trace_lane_scratch_bytes(const SqairHandle* h, int B, int K);   /* -1: bad arguments (K outside 1..256) */
int sqair_history_trace_lane(SqairHandle* h, void* ring, const int32_t* src_next, int lag, const SqairTraceOutputs* out,
                             const float* log_w /*[R] or NULL: uniform*/, const SqairTraceLane* lane, void* scratch,
                             int64_t scratch_bytes, void* stream);
/* Kernel-level check of the lane tracks (tests): the two lane kernels on caller tensors, no ring and no trace, any K in 1..256, the
 * handle's N, H, W.  where [F,B*K,N,4], presence, obj_id [F,B*K,N]: the traced rows, frames oldest -> newest; valid [F,B*K] int32;
 * log_w [B*K] or NULL.  Refused (return -1, before any HIP call): a NULL where / presence / obj_id / valid / lane / scratch, F (1 ..
 * 65535), B or K out of range, what lane refuses, scratch_bytes < sqair_trace_lane_scratch_bytes(h, B, K). */
int sqair_track_lane_test(SqairHandle* h, const float* where, const float* presence, const float* obj_id, const int32_t* valid,
                          const float* log_w, int F, int B, int K, const SqairTraceLane* lane, void* scratch, int64_t scratch_bytes,
                          void* stream);

/* ---- forecasting: the generative prior rolled forward from a carried state ------------------------------------------------
 * A forecast of F frames starts from the rows the NEXT pass would start from: state_in of sqair_set_state gathered through a source
 * map (src_rows, or the map given to sqair_set_state when NULL; -1 = the fresh initial state, as a pass's import).  Frame f = 0..F-1
 * is the reference's generated frame (seq.py:198-200, sqair_modules.py:157-170, :294-302) with discovery empty:
 *   (where_loc, where_scale, what_loc, what_scale, logit), prior_state' = PropagatePrior(z_{t-1}, prior_state)
 *       (prop_prior_type rnn / rw / guided as in the generation modes);
 *   where = where_loc + where_scale * eps[0:4], what = what_loc + what_scale * eps[4:4+n_what], presence = u < sigmoid(logit)
 *       with eps / u entry k of noise slot s = 0 of the frame (the forward pass's noise layout; s = 1 is not read);
 *   the record carried to the next frame holds presence_logit = that prior logit and presence_prob = sigmoid(logit);
 *   ids and compaction are the reference's merge with nothing discovered: compute_object_ids(last_id, prev_ids, presence, 0), then
 *       the N slots present-first in a stable order, each with its new prior state; last_id does not change;
 *   the decoder renders canvas mean and glimpses of the frame (no likelihood: there is no observation).
 * A forecast writes nothing but `out` and its own workspace: not the state blob, the source map, SMC buffers or any forward
 * workspace, so it may interleave with passes.  It is capturable (sqair_capture_begin / _end): no host sync, no allocation.
 * Summaries per lane b (SMC-weighted predictive): w_k = softmax over the lane's K entries of log_w (NULL: uniform),
 *   mean_canvas[f, b] = sum_k w_k canvas[f, b*K + k], expected_count[f, b] = sum_k w_k (present slots of particle k), sums over k in
 *   index order (the same bits on every replay).  A lane whose log weights hold a NaN or +inf, or are all -inf, gets NaN summaries.
 * Refused (return -1, text in sqair_last_error, before any HIP call): no state with state_in set, a B other than the state's,
 * F < 1, NULL noise, workspace_bytes < sqair_forecast_workspace_bytes(h, F, B), a configuration with sample_from_prior. */
typedef struct SqairForecastOutputs {   /* every pointer optional */
  float* what;            /* [F,B',N,n_what] */
  float* where;           /* [F,B',N,4] */
  float* presence;        /* [F,B',N] */
  float* presence_prob;   /* [F,B',N] sigmoid of the prior logit */
  float* presence_logit;  /* [F,B',N] */
  float* obj_id;          /* [F,B',N] */
  float* canvas;          /* [F,B',H,W] decoder mean */
  float* glimpse;         /* [F,B',N,G,G] */
  const float* log_w;     /* [B'] in: particle log weights for the summaries; NULL = uniform */
  float* mean_canvas;     /* [F,B,H,W]  sum_k w_k canvas_k,  w = softmax over the lane's K log weights */
  float* expected_count;  /* [F,B]      sum_k w_k * (objects present in particle k) */
} SqairForecastOutputs;
int64_t sqair_forecast_workspace_bytes(const SqairHandle* h, int F, int B);
int sqair_forecast(SqairHandle* h, const float* flat_params, const void* packed, const float* noise /*[F,B',2,N,nzw]*/,
                   int F, int B, const int32_t* src_rows /*NULL: the map of sqair_set_state*/,
                   const SqairForecastOutputs* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- object forecasts: fanned-out rollouts and one predictive answer per object of a lane -------------------------------------
 * sqair_forecast draws ONE rollout per particle row and answers per row; with K = 1 the predictive "distribution" is a single draw.
 * sqair_forecast_fan rolls every particle row forward S times inside one call, and, with `lane` set, turns the K*S rollouts of a
 * lane into one answer per object of the lane: predicted box, spread and survival mass per horizon, and the predictive count
 * distribution -- formed on the device, no host round trip, capturable like sqair_forecast, and with its promise: nothing but `out`,
 * `lane` and the workspace is written.  sqair_forecast is the S = 1, lane = NULL case of the same code and keeps its bits.
 * Fan-out.  R = B*K.  Rollout row q = r*S + s (r = b*K + k, s = 0..S-1) starts from exactly the row sqair_forecast starts row r
 *   from: the blob through src_rows[r] (the registered map when NULL); -1 or an index outside [0, R) gives the fresh initial state
 *   (the map is expanded into the workspace, src_fan[q] = src[q / S], the range rule applied against the blob's R).
 *   noise is [F, R*S, 2, N, nzw]; the per-row outputs of SqairForecastOutputs are read with B' = R*S; out->log_w stays [R];
 *   mean_canvas / expected_count stay [F, B, ...]: row q carries weight w_k / S (w = the lane's softmax as in sqair_forecast, the
 *   division in fp32), the sums run over the lane's K*S rows q in index order.
 * Lane forecast (SqairForecastLane; every pointer optional except best_row).  Per lane b:
 * 1. Weights and best row: sqair_set_estimate's points 1-2 on out->log_w alone (no per-frame terms; NULL: uniform), the same device
 *    helpers: weights[b,k] = w_k, best_row[b] = b*K + the first k of maximal log weight.
 * 2. start_where / start_presence / start_obj_id [R,N,.]: the frame-0 (imported) records of every particle row, 32-bit words
 *    copied.  The lane's objects are the best START row's slots j: presence, obj_id [B,N] copied words, box0 [B,N,4] = (y, x, h, w)
 *    in pixels as sqair_set_estimate's point 4; zero where the slot is absent.  A fresh best row has no present slot: no objects.
 * 3. Association, ONCE, on the start rows, by sqair_set_estimate's point 5: per object j and particle k, m* = the first present
 *    slot of k's start row of maximal IoU with box0[j]; k is associated with j when that IoU >= iou_min (not one-to-one).
 *    support[b,j] = sum_k w_k [k associated].  The obj_id word of slot m* is the id FOLLOWED in each of particle k's S rollouts: a
 *    forecast discovers nothing, so a survivor keeps its id while compaction moves it between slots.
 * 4. Per frame f and object j, over the rollouts q = (k, s) of the lane with k associated and a present slot of frame f whose obj_id
 *    word equals the followed id (an exact compare; the first such slot), weight w_q = w_k / S:
 *      alive[f,b,j]    = sum w_q                              (unnormalised: <= support, non-increasing in f)
 *      box_mean[f,b,j] = sum w_q box_q / alive                (box_q: the pixel box of that slot)
 *      box_std[f,b,j]  = sqrt(sum w_q (box_q - box_mean)^2 / alive)     (two passes in fp32: the mean first)
 *    Where alive is 0 the box statistics are NaN (0 / 0: nothing to average, and the value stays visible).  An absent best-row slot
 *    gives zeros in support, alive, box_mean, box_std.
 * 5. count_prob[f,b,c] = sum_q w_q [rollout q holds c present slots at frame f], c = 0..N.
 * 6. Every sum over rollouts is ONE thread's loop over q in index order (over k for support): fixed by (K, S) alone, no float
 *    atomics, the same bits eager or replayed from a graph.
 * 7. Non-finite lanes, sqair_set_estimate's point 7: a NaN or +inf log weight, or all of them -inf, gives NaN weights, support,
 *    alive, box_mean, box_std and count_prob, best_row = -1 and no objects (presence, obj_id, box0 zero).
 * Refused (return -1, text in sqair_last_error, before any HIP call): everything sqair_forecast refuses; S < 1; K*S >
 * SQAIR_FORECAST_FAN_MAX (the rollouts of a lane are staged in LDS, one 16-byte box each); R*S*N beyond int32; workspace_bytes <
 * sqair_forecast_fan_workspace_bytes(h, F, B, S) (>= sqair_forecast_workspace_bytes(h, F, B) at S = 1); with lane set: iou_min NaN or
 * outside (0, 1], a NULL best_row. */
#define SQAIR_FORECAST_FAN_MAX 1024
typedef struct SqairForecastLane {
  float iou_min;             /* in (0, 1] */
  int32_t* best_row;         /* [B] required */
  float* weights;            /* [B,K] */
  float* start_where;        /* [R,N,4] */
  float* start_presence;     /* [R,N] */
  float* start_obj_id;       /* [R,N] */
  float* obj_id;             /* [B,N] */
  float* presence;           /* [B,N] */
  float* box0;               /* [B,N,4] (y, x, h, w) in pixels */
  float* support;            /* [B,N] */
  float* alive;              /* [F,B,N] */
  float* box_mean;           /* [F,B,N,4] */
  float* box_std;            /* [F,B,N,4] */
  float* count_prob;         /* [F,B,N+1] */
} SqairForecastLane;
int64_t sqair_forecast_fan_workspace_bytes(const SqairHandle* h, int F, int B, int S);
int sqair_forecast_fan(SqairHandle* h, const float* flat_params, const void* packed, const float* noise /*[F,R*S,2,N,nzw]*/,
                       int F, int B, int S, const int32_t* src_rows /*[R] or NULL: the map of sqair_set_state*/,
                       const SqairForecastOutputs* out, const SqairForecastLane* lane /*NULL: none*/, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* Kernel-level check of the lane forecast (tests): the same kernels on caller tensors, no state and no forecast, any K in 1..256 and
 * S with K*S <= SQAIR_FORECAST_FAN_MAX, the handle's N, H, W.  start_where [B*K,N,4], start_presence, start_obj_id [B*K,N]: the start
 * rows; where [F,B*K*S,N,4], presence, obj_id [F,B*K*S,N]: the rollouts; log_w [B*K] or NULL.  scratch: device memory of
 * sqair_forecast_lane_scratch_bytes(h, B, K) bytes (the weights, the association and the followed ids between the two launches).
 * Refused (return -1, before any HIP call): a NULL start_* / where / presence / obj_id / lane / scratch, F, B, K or S out of range,
 * what lane refuses, scratch_bytes too small. */
int64_t sqair_forecast_lane_scratch_bytes(const SqairHandle* h, int B, int K);
int sqair_forecast_lane_test(SqairHandle* h, const float* start_where, const float* start_presence, const float* start_obj_id,
                             const float* where, const float* presence, const float* obj_id, const float* log_w, int F, int B, int K,
                             int S, const SqairForecastLane* lane, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- missing-frame steps: unobserved lanes coast on the prior, inside the pass ------------------------------------------------
 * Cameras drop frames, lanes of a batch run at different rates, an object passes behind an occluder the caller knows about.  With
 * a mask set, every following inference pass with a carried state reads observed[T, B] (device int32, nonzero = the lane has a
 * frame) ON THE DEVICE, so one captured graph serves every pattern of present and missing lanes.  For an observed (frame, lane)
 * nothing changes, bit for bit.  For an unobserved (frame t, lane b) each of the lane's K rows takes a COASTED frame, the
 * particle filter's treatment of a missing observation -- propose from the transition prior, leave the weight alone, let time
 * advance:
 *   records and ids: what / where / presence / presence_logit / presence_prob / obj_id of frame t are exactly the frame
 *       sqair_forecast would produce from the rows of t - 1 (the same device code: PropagatePrior, the draws from noise slot s = 0 of
 *       the frame's ordinary noise -- s = 1 is not read --, compute_object_ids with nothing discovered, the N slots present-first
 *       in a stable order); last_id does not move;
 *   prior state: each slot's new prior-cell state travels with it, as in the forecast;
 *   temporal state: HELD (no glimpse, no update) and carried with its slot through the same permutation -- the reference's merge,
 *       select_present over [temporal_prev | init_temporal] with discovery absent; an LSTM state moves as [h | c];
 *   the row's frame counter advances as for any frame: a coasted frame is time that passed;
 *   log_weights_per_timestep = 0, so a coasted frame changes neither the accumulated log weights, nor the ESS, nor log_evidence;
 *   canvas and glimpse are the decoder's render of the coasted records;
 *   num_prop_steps_per_sample = num_steps_per_sample = the number of present slots, num_disc_steps_per_sample = 0, prop_pres = the
 *       compacted presence, disc_pres = 0;
 *   every other bound SqairOutputs buffer is written as 0 for that (frame, row): the posterior locs and scales, all *_log_prob,
 *       disc_prob, prop_prob, step_log_prob, discrete_log_prob, data_ll_per_sample, kl_per_sample, log_q_z_given_x_per_sample,
 *       log_p_z_per_sample.
 * The frame of an unobserved lane influences no output and no state word, but it must be FINITE: the pass still computes on it
 * (the posterior runs on every row; the step is bound by its dependent launches, not its rows).  Within a pass of T > 1 frames the
 * mask is per frame: frame t + 1 of a lane reads the coasted frame t.  A pass with a mask has exactly T + 1 kernel nodes more
 * (k_coast_step after each frame's compaction, k_coast_finish before the state export, the history push and the resampler, so the
 * history records the coasted outputs and the resampler reads zero log weights); without one nothing is launched.
 * The pointer is remembered by the handle and frozen into captured graphs, as the state's pointers are.  NULL observed: off.
 * Refused (return -1, text in sqair_last_error, before any HIP call): no state set, T < 1, a B other than the state's, a
 * configuration with sample_from_prior; at pass time: a pass whose T is not the T given here, and every training call
 * (sqair_forward_train, sqair_forward_train_carry) while a mask is set -- training on gappy streams is out of scope for THIS mask,
 * which belongs to the handle's inference state: a carried training chunk takes its mask per call, sqair_forward_train_carry_masked /
 * sqair_backward_carry_masked below ("training on gappy and ragged streams").
 * sqair_set_state switching the state off, or to another B, switches the mask off. */
int sqair_set_observed(SqairHandle* h, const int32_t* observed /* device [T,B]; NULL: off */, int T, int B);

/* ---- lane estimates: one answer per lane from its K particles, inside the pass ----------------------------------------------
 * A pass returns K particle rows per lane; a tracker's caller wants one answer per camera: how many objects, where (boxes in
 * pixels), how sure.  With an estimate set, every following inference pass with a carried state ends with one more kernel,
 * k_lane_estimate, one workgroup per (lane b, frame t): after k_coast_finish, the state export and the history push, and BEFORE the
 * SMC resampler, which zeroes log_w and rewrites the source map.  No host round trip: one captured graph serves every step.  A
 * pass with the estimate on has exactly one kernel node more; with it off nothing is launched and every other output, blob and
 * accumulator is unchanged bit for bit.  Training passes never run it.
 * For frame t of the pass and lane b, rows r = b*K + k:
 * 1. Weights.  a_k(t) = log_w[r] + sum over t' <= t of log_weights_per_timestep[t', r], in frame order, in fp32: the resampler's
 *    accumulation stopped at frame t.  m = max_k a_k, e_k = expf(a_k - m), S = sum e_k, w_k = e_k / S, ESS = S^2 / sum e_k^2, each
 *    sum one thread's loop in index order -- the device code of the resampler and of the forecast's summaries, not a restatement.
 *    weights[t,b,k] = w_k, ess[t,b] = ESS; with SMC on, ess[T-1, b] is the resampler's ess[b] bit for bit.  log_w is the carried
 *    log weight of this pass's rows, as it stands when the pass runs (with SMC: smc->log_w); NULL means zeros.
 * 2. Best row.  best_row[t,b] = b*K + the first k of maximal a_k (an exact compare: a_k is defined in fp32).
 * 3. Count posterior.  n_k = the number of present slots (presence != 0) of row k; count_prob[t,b,c] = sum_k w_k [n_k = c] for
 *    c = 0..N, expected_count[t,b] = sum_k w_k n_k, map_count[t,b] = the first c of maximal count_prob; k in index order.
 * 4. The lane's objects are the best row's slots j (already present-first): presence, obj_id [t,b,N], where [t,b,N,4] and what
 *    [t,b,N,n_what] are copies of the best row's 32-bit words, zero where the slot is absent.  box[t,b,j] = (y, x, h, w) in pixels
 *    is the reference's stn_to_pixel_coords(to_coords(where), (H, W)) (sqair/modules.py:221-262):
 *      (sx, sy, tx, ty) = to_coords(where) (sigmoid kept >= 1e-4, tanh), y = (H - 1) / 2 (ty - sy + 1), h = (H + 1) sy,
 *      x = (W - 1) / 2 (tx - sx + 1), w = (W + 1) sx,
 *    with the device to_coords of the crop and insert kernels: the box the decoder drew with.  Zero where absent.
 * 5. Support and consensus box, by SPATIAL association -- not by id: obj_id is a per-row counter that agrees between two rows
 *    only as far back as their common ancestor, and slots are not objects (compaction moves them).  For each present best-row
 *    object j and each particle k:  m* = the first present slot of row k with maximal IoU(box[j], box of (k, m)).  Boxes are axis
 *    aligned; IoU = intersection / union with overlap lengths min(y1 + h1, y2 + h2) - max(y1, y2) (x alike) clipped at 0; 0 when
 *    the union is not positive, else exactly 1 for two boxes with the same four words.  Particle k AGREES on j when that IoU >=
 *    iou_min.  support[t,b,j] = sum_k w_k [k agrees] (the best row always agrees with itself: its IoU is 1), box_mean[t,b,j] =
 *    sum_k w_k [k agrees] box of (k, m*) / support; both zero where slot j is absent.  k in index order: the same bits on every
 *    replay, eager or graph.  Matching is NOT one-to-one: two best-row objects may be matched by the same slot of a particle
 *    (one-to-one, Hungarian, matching is out of scope).
 * 6. mean_canvas[t,b] = sum_k w_k canvas[t, r], k in index order: only when asked for, and the pass must then bind out->canvas.
 * 7. Non-finite lanes: the resampler's rule, bad values stay visible.  A lane whose S is not finite (some a_k NaN or +inf, or
 *    every a_k -inf) gives NaN weights, ess, count_prob, expected_count, support, box_mean and mean_canvas, best_row = map_count
 *    = -1 and zero objects (presence, obj_id, where, what, box).  Finite lanes of the same launch are unaffected.
 * 8. Coasted (frame, lane)s (sqair_set_observed) need no special case: their records are the coasted ones, their log weight 0.
 * Every pointer of SqairLaneEstimate is optional except best_row.  Pointers are remembered by the handle and frozen into captured
 * graphs, as the state's are.  NULL est: off.  Refused (return -1, text in sqair_last_error, before any HIP call): no state set,
 * T < 1, a B other than the state's, iou_min NaN or outside (0, 1], a NULL best_row, with SMC on a log_w other than smc->log_w;
 * at pass time: a pass of another T, a NULL out->log_weights_per_timestep, mean_canvas without out->canvas, SMC on with another
 * log_w.  The objects are read from the pass's own merged slot records, not from its SqairOutputs buffers: those need not be
 * bound.  sqair_set_state switching the state off, or to another B, switches the estimate off.
 * Out of scope: estimates for training passes.  Smoothed (lagged) estimates are sqair_history_trace_lane's: one trajectory per object
 * of a lane from the K traced paths. */
typedef struct SqairLaneEstimate {
  float iou_min;             /* in (0, 1] */
  const float* log_w;        /* [B*K] in: carried log weights of the pass's rows; NULL = zeros */
  int32_t* best_row;         /* [T,B] required */
  float* weights;            /* [T,B,K] */
  float* ess;                /* [T,B] */
  float* count_prob;         /* [T,B,N+1] */
  float* expected_count;     /* [T,B] */
  int32_t* map_count;        /* [T,B] */
  float* presence;           /* [T,B,N] */
  float* obj_id;             /* [T,B,N] */
  float* where;              /* [T,B,N,4] */
  float* what;               /* [T,B,N,n_what] */
  float* box;                /* [T,B,N,4] (y, x, h, w) in pixels */
  float* support;            /* [T,B,N] */
  float* box_mean;           /* [T,B,N,4] */
  float* mean_canvas;        /* [T,B,H,W] */
} SqairLaneEstimate;
int sqair_set_estimate(SqairHandle* h, const SqairLaneEstimate* est /* NULL: off */, int T, int B);
/* Kernel-level check of the estimate (tests): the kernel above on caller buffers, no state and no pass, any K in 1..256 with the
 * handle's N, n_what, H, W.  where [T,B*K,N,4], presence, obj_id [T,B*K,N], what [T,B*K,N,n_what] (or NULL), canvas [T,B*K,H,W]
 * (or NULL), lw [T,B*K] standing for the pass's log_weights_per_timestep.  Refused (return -1, before any HIP call): a NULL where /
 * presence / obj_id / lw / est, T, B or K out of range, what est refuses, est->what without what, est->mean_canvas without canvas. */
int sqair_lane_estimate_test(SqairHandle* h, const float* where, const float* presence, const float* obj_id, const float* what,
                             const float* canvas, const float* lw, int T, int B, int K, const SqairLaneEstimate* est, void* stream);

/* ---- object layers: per-object appearance, coverage and pixel owners of a lane, inside the pass --------------------------------
 * The estimate says how many objects a lane holds and where; the layers say which pixels each of them occupies and what it looks
 * like there: the object's segmentation and its appearance on the frame.  The decoder draws the canvas as a sum over slots of
 * inverse-warped glimpses plus a written-to mask; the layers are that sum taken apart per object of the lane.  With layers set, every
 * following inference pass with a carried state and an estimate runs one more kernel, k_lane_layers, directly after
 * k_lane_estimate and BEFORE the SMC resampler, which zeroes the weights.  A pass with layers on has exactly one kernel node more;
 * with layers off nothing is launched and every other output, blob and accumulator is unchanged bit for bit.  Training passes never
 * run it.  It reads the pass's own decoded glimpses and merged slot records: neither needs to be bound as an output.
 * For frame t of the pass, row r and slot m with where logits wl, presence p and decoded glimpse g [G, G], two images [H, W]:
 *   V(r, m) = p * (inverse spatial transformer of g),  O(r, m) = p * (inverse spatial transformer of a glimpse of ones)
 * -- what the decoder adds into its canvas and its written-to mask for that slot, by the decoder's own device functions
 * (sq_canvas_coord, sq_canvas_tap, the to_coords of the crop and insert kernels); a pixel outside the slot's box receives exactly 0.
 * For lane b, rows r = b*K + k:
 * 1. Shared quantities.  The weights w_k, the best row, the best row's objects j and the association of every particle with them are
 *    sqair_set_estimate's points 1, 2, 4 and 5, computed by the same device functions, with the estimate's iou_min and log_w.
 * 2. match[t,b,k,j] (int32) = the slot m* of particle k associated with best-row object j; -1 when k does not agree on j, when j is
 *    absent, or when the lane is non-finite.  It is the table the estimate builds for its support: with it a caller gathers any
 *    per-row output per object of the lane.
 * 3. For each present j, A_j = {k : match[t,b,k,j] >= 0} and s_j = sum over A_j of w_k -- the estimate's support, summed in the same
 *    order.  layer[t,b,j] = sum over A_j of w_k V(b*K + k, match[t,b,k,j]) / s_j, cover[t,b,j] the same with O: [H, W] in fp32, k in
 *    index order, one thread per pixel, no float atomics: the same bits on every replay, eager or graph.  Absent j: zeros.  The best
 *    row always agrees with itself, so s_j >= w_best > 0: a convex combination.
 * 4. owner[t,b,y,x] (int32) = the first present j of maximal cover[t,b,j,y,x] if that maximum is >= cover_min, else -1
 *    (background).  A NaN never wins.
 * 5. Non-finite lanes follow the estimate's rule 7: layer and cover are NaN, match and owner -1; finite lanes of the same launch
 *    are unaffected.
 * 6. Coasted (frame, lane)s need no special case: the decoder ran on their coasted records.
 * 7. Consequence.  At K = 1, layer[j] = V(best, j), so sum_j layer[j] + mean_img * sigmoid(-10 + 20 sum_j cover[j]) is the pass's own
 *    canvas of that row.
 * Every pointer of SqairLaneLayers is optional, at least one must be set; owner needs no cover bound.  Pointers are remembered by the
 * handle and frozen into captured graphs.  NULL lay: off.  Refused (return -1, text in sqair_last_error, before any HIP call): no
 * estimate set (sqair_set_estimate), a T other than the estimate's, a B other than the state's, cover_min NaN or outside (0, 1], all
 * four pointers NULL; at pass time: a pass of another T.  sqair_set_estimate switching the estimate off or to another T, and
 * sqair_set_state switching the state off or to another B, switch the layers off.
 * Out of scope: layers of forecasts and of lane tracks, per-particle-row layers, one-to-one matching, layers for training passes. */
typedef struct SqairLaneLayers {
  float cover_min;           /* in (0, 1] */
  int32_t* match;            /* [T,B,K,N] */
  float* layer;              /* [T,B,N,H,W] */
  float* cover;              /* [T,B,N,H,W] */
  int32_t* owner;            /* [T,B,H,W] */
} SqairLaneLayers;
int sqair_set_layers(SqairHandle* h, const SqairLaneLayers* lay /* NULL: off */, int T, int B);
/* Kernel-level check of the layers (tests): the kernel above on caller buffers, no state and no pass, any K in 1..256 with the
 * handle's N, G, H, W.  glimpse [T,B*K,N,G,G], where [T,B*K,N,4], presence [T,B*K,N], lw [T,B*K] standing for the pass's
 * log_weights_per_timestep, log_w [B*K] or NULL (zeros).  Refused (return -1, before any HIP call): a NULL glimpse / where / presence
 * / lw / lay, T, B or K out of range, iou_min NaN or outside (0, 1], what sqair_set_layers refuses for lay. */
int sqair_lane_layers_test(SqairHandle* h, const float* glimpse, const float* where, const float* presence, const float* lw,
                           const float* log_w, float iou_min, int T, int B, int K, const SqairLaneLayers* lay, void* stream);

/* ---- stream scoring: CLEAR-MOT events of the lane answer against ground-truth boxes, inside the pass ---------------------------
 * The estimate, the layers, the lane tracks and the lane forecasts say what the filter believes; the score says whether the lane
 * answer follows the objects of the scene and whether obj_id stays on them.  The lane's obj_id is the best row's, and ids agree
 * between rows only back to their common ancestor: a switch of the best row can switch the identity the caller sees -- an identity
 * switch below.  With a score set, every following inference pass with a carried state and an estimate runs one more kernel,
 * k_lane_score, one workgroup per lane looping over the pass's frames in order: after k_lane_estimate (and after k_lane_layers if
 * on) and BEFORE the SMC resampler.  A pass with the score on has exactly one kernel node more; with the score off nothing is
 * launched and every other output, blob and accumulator is unchanged bit for bit.  Training passes never run it.  The kernel reads
 * the estimate's own output buffers box, presence, obj_id and map_count -- they must be bound -- and does not read the records again.
 * Inputs per pass, on the device, read by the kernel so that one captured graph serves every pattern: truth_box [T,B,G,4] fp32
 * (y, x, h, w) in pixels, the convention of the estimate's box; truth_present [T,B,G] int32 -- truth identity IS the slot g: an
 * object keeps its slot for its life; truth_valid [T,B] int32, 0 = this (frame, lane) has no truth: it is not scored and leaves the
 * memory and the accumulators untouched.  G in 1..16 is chosen when the score is set.
 * For lane b and the frames t of the pass in order with truth_valid[t,b] != 0:
 * 0. Non-finite lanes.  The estimate's non-finite lane (map_count == -1) counts one frames_invalid and nothing else changes.  For
 *    such a frame, and for a frame without truth, the per-frame outputs are -1 (truth_match, tp, fn, fp, idsw) and 0 (match_iou).
 * 1. Candidates: present truth g (truth_present != 0) x present lane object j (presence != 0).  Holes are allowed on both sides:
 *    nothing is assumed present-first.  IoU(g, j) is the estimate's (point 5 above: the same device function, sq_box_iou, on the
 *    fp32 words).
 * 2. Keep.  last_id[b,g] is the identity memory: the obj_id WORD (the 32 bits of the float, read as int32) of the lane object truth
 *    g was last matched with, -1 = none yet; a negative word (a negative id: the model makes none) is stored as it is and then
 *    reads as no memory.  For g in index order with last_id[b,g] >= 0: the first unclaimed present j whose obj_id word equals
 *    last_id[b,g] and whose IoU(g, j) >= iou_min is matched with g and claimed.
 * 3. Rest: greedy one-to-one.  Repeat: among unmatched present g and unclaimed present j with IoU >= iou_min take the pair of
 *    maximal IoU, ties to the smallest g, then the smallest j; stop when no such pair is left.  A NaN never wins.
 * 4. Events.  tp[t,b] = matched pairs, fn[t,b] = present truths unmatched, fp[t,b] = present lane objects unclaimed.  For each
 *    matched g in index order with id = the obj_id word of its j: idsw[t,b] += [last_id[b,g] >= 0 and last_id[b,g] != id], then
 *    last_id[b,g] = id; unmatched g keep their memory.  match_iou[t,b,g] = the pair's IoU (0 unmatched), truth_match[t,b,g] = j
 *    (-1 unmatched or absent).  With n_truth = the number of present truths: count_hit += [map_count == n_truth], count_abs_err
 *    += |map_count - n_truth|.
 * 5. Accumulators persist across passes and are updated in place -- read, added to, written by one thread -- so a replayed graph
 *    accumulates as eager calls do.  counts [B,9] int64: frames (scored), frames_invalid, truth, tp, fn, fp, idsw, count_hit,
 *    count_abs_err.  iou_sum [B] fp64 += match_iou[t,b,g] converted to fp64, g in index order, frames in order, from one thread:
 *    no float atomics, the same bits eager and graph.  The caller zeroes counts and iou_sum and sets last_id to -1 to start.
 * 6. Coasted (frame, lane)s (sqair_set_observed) need no case of their own: they are scored when their truth is valid.
 * Pointers are remembered by the handle and frozen into captured graphs.  NULL score: off.  Refused (return -1, text in
 * sqair_last_error, before any HIP call): no estimate set (sqair_set_estimate); an estimate without box, presence, obj_id or
 * map_count; a T other than the estimate's, a B other than the state's; G outside 1..16; iou_min NaN or outside (0, 1]; a NULL
 * truth_box, truth_present, truth_valid, counts, iou_sum or last_id (the per-frame outputs are optional); at pass time: a pass
 * of another T.  sqair_set_estimate switching the estimate off, to another T or to one without the four fields, and
 * sqair_set_state switching the state off or to another B, switch the score off.
 * Out of scope: optimal (Hungarian) assignment per frame -- step 3 is greedy (IDF1 and the mostly-tracked / mostly-lost statistics,
 * with the optimal assignment over a clip they need, are sqair_set_idf's, below) here: step 3 as keep + optimal is
 * sqair_set_lane_match's, below; scoring per particle row;
 * scoring of forecasts or lane tracks; training passes. */
#define SQAIR_SCORE_MAX_TRUTH 16
#define SQAIR_SCORE_COUNTS 9
typedef struct SqairLaneScore {
  float iou_min;                  /* in (0, 1] */
  int32_t G;                      /* truth slots per lane, 1..16 */
  const float* truth_box;         /* [T,B,G,4] in */
  const int32_t* truth_present;   /* [T,B,G] in */
  const int32_t* truth_valid;     /* [T,B] in */
  int64_t* counts;                /* [B,9] in/out */
  double* iou_sum;                /* [B] in/out */
  int32_t* last_id;               /* [B,G] in/out */
  int32_t* truth_match;           /* [T,B,G] */
  float* match_iou;               /* [T,B,G] */
  int32_t* tp;                    /* [T,B] */
  int32_t* fn;                    /* [T,B] */
  int32_t* fp;                    /* [T,B] */
  int32_t* idsw;                  /* [T,B] */
} SqairLaneScore;
int sqair_set_score(SqairHandle* h, const SqairLaneScore* score /* NULL: off */, int T, int B);
/* Kernel-level check of the score (tests): the kernel above on caller buffers, no state and no pass, with the handle's N and any G
 * in 1..16.  box [T,B,N,4], presence, obj_id [T,B,N] and map_count [T,B] stand for the estimate's outputs.  Refused (return -1,
 * before any HIP call): a NULL box / presence / obj_id / map_count / score, T or B out of range, what sqair_set_score refuses for
 * score. */
int sqair_lane_score_test(SqairHandle* h, const float* box, const float* presence, const float* obj_id, const int32_t* map_count,
                          int T, int B, const SqairLaneScore* score, void* stream);
/* Forecasts and lane tracks are scored by sqair_lane_traj_score, next. */

/* ---- trajectory scoring: a lane forecast or a lane track table against the truth's trajectories ------------------------------
 * The score above checks the lane's answer about the present.  sqair_lane_traj_score checks the two answers that reach over time --
 * the lane forecast (SqairForecastLane, the future) and the lane tracks (SqairTraceLane, the past) -- against ground-truth boxes, on
 * the device: does the predicted box land on the object f frames on, is alive / support an honest survival probability, how far is the
 * smoothed box from where the object was.  Both tables list the same objects in the same layout, so one scorer serves both.  It is a
 * stand-alone, capturable call: neither registered on the handle nor part of a pass; it runs after sqair_forecast_fan or
 * sqair_history_trace_lane on the table either of them wrote (or on a caller's tensors: it is its own kernel-level entry), one launch
 * of k_lane_traj_score.  The handle gives N and the error text only; it reads the table and the truth and writes only `score`.
 * The table (SqairLaneTraj, read-only) holds the fields SqairForecastLane and SqairTraceLane share: best_row [B], presence, obj_id,
 * support [B,N], box0 [B,N,4], alive [F,B,N], box_mean [F,B,N,4], count_prob [F,B,N+1], and valid_mass [F,B] (NULL: mass 1 everywhere,
 * the forecast's case).  The truth (SqairTrajTruth): G in 1..16 slots per lane, truth identity IS the slot g as in sqair_set_score;
 * the ANCHOR -- anchor_box [B,G,4], anchor_present [B,G], anchor_valid [B] -- is the truth at the frame the table's objects are read
 * from, the last stepped frame (frame F-1 of lane tracks, the frame before f = 0 of a forecast); truth_box [F,B,G,4], truth_present
 * [F,B,G], truth_valid [F,B] are the truth at the table's frames.  Boxes are fp32 (y, x, h, w) in pixels, masks int32 (nonzero = set).
 * For each lane b:
 * 0. Lane not scored.  anchor_valid[b] == 0: the lane is untouched -- no accumulator changes, the per-call outputs are -1 (integers)
 *    and 0 (floats).  A valid anchor on a non-finite lane (best_row[b] == -1) counts one calls_invalid and changes nothing else; the
 *    per-call outputs are -1 and 0 as well.
 * 1. Link, once per call.  Candidates: anchor-present truth g x present lane object j (presence != 0); holes are allowed on both
 *    sides.  IoU(g, j) = sq_box_iou(anchor_box[b,g], box0[b,j]), the estimate's device function on the fp32 words.  The assignment is
 *    sq_assign_keep_greedy, the score's device function, unchanged (points 2 and 3 above: keep, then greedy one-to-one, ties to the
 *    smallest g, then the smallest j; a NaN never wins), with iou_min, and with keep_id[b,g] against the obj_id words when keep_id is
 *    given (a scorer's last_id: the truth stays with the identity it was last matched with).  link[b,g] = j or -1, link_iou[b,g] =
 *    the pair's IoU (0 unlinked).  lane_counts[b,:] += (calls, calls_invalid, anchor_truth, linked): calls = 1 for a scored lane,
 *    anchor_truth = the anchor-present truths, linked = those with link >= 0.
 * 2. Per frame f that is scored -- truth_valid[f,b] != 0 and valid_mass[f,b] > 0 (a NULL valid_mass counts as positive) -- and each g
 *    with j = link[b,g] >= 0:  p_alive[f,b,g] = p = alive[f,b,j] / support[b,j], an fp32 division; y = [truth_present[f,b,g] != 0];
 *    brier = (p - y)^2 in fp32.
 *      state 1, a pair: y and alive[f,b,j] > 0.  pair_iou[f,b,g] = sq_box_iou(truth_box[f,b,g], box_mean[f,b,j]); centre_err[f,b,g] =
 *               the Euclidean distance in pixels between the two box centres (y + h/2, x + w/2), in fp32; hits += [pair_iou >= iou_min].
 *      state 2, lost: y and alive[f,b,j] not positive -- the filter's paths do not hold a living object; a NaN box_mean is never read.
 *      state 0, gone: not y.  Only the Brier term counts.
 *    An unlinked g, or a frame that is not scored, gives state[f,b,g] = -1 and zeros (p_alive, pair_iou, centre_err).
 * 3. Count, per scored frame.  count_map[f,b] = the first argmax of count_prob[f,b,:] (-1 for a frame not scored); n_truth = the
 *    number of present truths of the frame, linked or not; count_hit += [count_map == n_truth], count_abs_err += |count_map - n_truth|.
 * 4. Accumulators, per (frame, lane): counts[f,b,:] int64 = (frames, pairs, hits, lost, gone, count_hit, count_abs_err); sums[f,b,:]
 *    fp64 = (iou_sum, centre_err_sum, brier_sum): each fp32 value converted to fp64 and added to the cell, g in index order.  They are
 *    updated in place: one thread owns each cell (f, b) -- it reads, adds and writes; no float atomics -- so a replayed graph
 *    accumulates the bits eager calls do.  The caller zeroes counts, sums and lane_counts to start.
 * 5. Refused (return -1, text in sqair_last_error, before any HIP call): a NULL table, truth or score; a NULL best_row, presence,
 *    support, box0, alive, box_mean, count_prob, anchor_box, anchor_present, anchor_valid, truth_box, truth_present, truth_valid,
 *    counts, sums or lane_counts (obj_id, valid_mass, keep_id and the per-call outputs are optional); F outside 1..65535 or B < 1; G
 *    outside 1..16; iou_min NaN or outside (0, 1]; a keep_id without a table obj_id.
 * 6. Out of scope: optimal (Hungarian) assignment -- the link is greedy here; the link as keep + optimal is sqair_set_lane_match's,
 *    below; calibration of box_std; trajectory scoring per particle
 *    row; truth for departed objects (the tables list the objects of the last stepped frame only); a truth ring kept by the stream --
 *    the caller brings the truth of the table's frames. */
#define SQAIR_TRAJ_COUNTS 7
#define SQAIR_TRAJ_SUMS 3
#define SQAIR_TRAJ_LANE_COUNTS 4
typedef struct SqairLaneTraj {
  const int32_t* best_row;        /* [B] */
  const float* presence;          /* [B,N] */
  const float* obj_id;            /* [B,N]; NULL allowed without keep_id */
  const float* support;           /* [B,N] */
  const float* box0;              /* [B,N,4] */
  const float* alive;             /* [F,B,N] */
  const float* box_mean;          /* [F,B,N,4] */
  const float* count_prob;        /* [F,B,N+1] */
  const float* valid_mass;        /* [F,B]; NULL = 1 everywhere */
} SqairLaneTraj;
typedef struct SqairTrajTruth {
  int32_t G;                      /* truth slots per lane, 1..16 */
  const float* anchor_box;        /* [B,G,4] */
  const int32_t* anchor_present;  /* [B,G] */
  const int32_t* anchor_valid;    /* [B] */
  const float* truth_box;         /* [F,B,G,4] */
  const int32_t* truth_present;   /* [F,B,G] */
  const int32_t* truth_valid;     /* [F,B] */
  const int32_t* keep_id;         /* [B,G]; NULL = no keep */
} SqairTrajTruth;
typedef struct SqairTrajScore {
  float iou_min;                  /* in (0, 1] */
  int64_t* counts;                /* [F,B,7] in/out */
  double* sums;                   /* [F,B,3] in/out */
  int64_t* lane_counts;           /* [B,4] in/out */
  int32_t* link;                  /* [B,G] */
  float* link_iou;                /* [B,G] */
  int32_t* state;                 /* [F,B,G] */
  float* p_alive;                 /* [F,B,G] */
  float* pair_iou;                /* [F,B,G] */
  float* centre_err;              /* [F,B,G] */
  int32_t* count_map;             /* [F,B] */
} SqairTrajScore;
int sqair_lane_traj_score(SqairHandle* h, const SqairLaneTraj* table, const SqairTrajTruth* truth, const SqairTrajScore* score, int F,
                          int B, void* stream);

/* ---- lane identities: stable per-lane track ids, formed inside the pass --------------------------------------------------------
 * The lane's obj_id is the best row's per-row counter: a switch of the best row switches the identity the caller sees although the
 * object did not move (the score's idsw counts exactly that), and an object the filter drops for a few frames comes back under a
 * fresh id.  With an identity set, every following inference pass with a carried state and an estimate runs one more kernel,
 * k_lane_identity, one workgroup per lane looping over the pass's frames in order: after k_lane_estimate (and after k_lane_layers if
 * on), BEFORE k_lane_score if on and BEFORE the SMC resampler.  It keeps a table of M tracks per lane on the device and links the
 * lane's objects to them frame by frame, so one captured graph serves every step.  A pass with the identity on has exactly one kernel
 * node more; with it off nothing is launched and every other output, blob and accumulator is unchanged bit for bit.  Training passes
 * never run it.  The kernel reads the estimate's own output buffers box, presence, obj_id, best_row (and what, when trk_what is
 * given) -- they must be bound -- and does not read the records again.
 * The memory, per lane b and entry e < M: trk_id (-1 = free; the other fields of a free entry are whatever they last held and are
 * never read), trk_word (the obj_id WORD -- the 32 bits of the float, read as int32 -- last seen on the track), trk_age (frames since
 * it was last seen), trk_len (frames it was seen in), trk_box (its last box, the estimate's four words), trk_what (its last what,
 * n_what words); next_id[b], the next fresh id of the lane.  The caller starts with trk_id = -1 and everything else 0.
 * For lane b and the frames t of the pass in order:
 * 0. Non-finite lane (best_row[t,b] == -1): lane_id, how and track_len are -1, frames_invalid += 1, the memory is untouched -- no
 *    ageing.
 * 1. Table.  For every entry e < M and slot j < N: IoU(e, j) = sq_box_iou(trk_box[e], box[t,b,j]) on the fp32 words (the estimate's
 *    point 5), or -1 when e is free (trk_id < 0) or j is absent (presence == 0).
 * 2. Link by position, the same lineage first: ONE call of sq_assign_keep_greedy, the device function of the score's points 2
 *    and 3, as it stands -- rows are the entries, columns the slots, keep_id[e] = trk_word[e] for live entries and -1 for free
 *    ones, col_id[j] = the obj_id word of slot j, a pair is eligible at IoU >= iou_min; keep, then greedy one-to-one, ties to the
 *    smallest e, then the smallest j; a NaN never passes.  For a matched pair how = 1 (kept) when trk_word[e] equals the word of j,
 *    else how = 2 (bridged: the caller would have lost the identity).
 * 3. Nothing else is done in the position link.
 * 4. Re-identification, only when reid_dist > 0.  For each still unmatched present j in index order, over the unclaimed live
 *    entries e: centres are (y + 0.5 h, x + 0.5 w), dc2 the squared centre distance, r = reid_dist * (trk_age[e] + 1); e is
 *    eligible when dc2 <= r * r and, with trk_what given, dw <= reid_what, where dw = (sum over c in index order of fmaf(d, d, acc),
 *    d = what[t,b,j,c] - trk_what[e][c]) / n_what in fp32, one thread's loop per pair.  A NaN never passes.  The eligible e of
 *    minimal dw is taken -- without trk_what the one of minimal dc2 --, ties to the smallest e; it is claimed and how = 3
 *    (re-identified).  Greedy in j on purpose: simple and reproducible.
 * 5. Update.  For a matched e (steps 2 and 4): trk_box, trk_word and trk_what become the 32-bit words of j, trk_age = 0,
 *    trk_len += 1; lane_id[t,b,j] = trk_id[e], track_len[t,b,j] = trk_len[e].
 * 6. Births, the remaining present j in index order: the first free entry, or if there is none the unclaimed live entry of largest
 *    trk_age, ties to the smallest e, which is evicted (ended += 1) -- M >= N guarantees that one exists.  trk_id = next_id[b],
 *    next_id[b] += 1, trk_len = 1, trk_age = 0, the words of j as in 5, how = 0 (born).  An entry freed or born in this frame is not
 *    a candidate of step 4 of the same frame: a birth follows every link.
 * 7. Ageing.  Every live entry neither matched nor born in this frame: trk_age += 1, and if that exceeds max_age the entry is freed
 *    (trk_id = -1) and ended += 1.
 * 8. Counters, counts [B,8] int64: frames, frames_invalid, objects (present slots seen), kept, bridged, reidentified, born (one count
 *    per value of how), ended.  Absent slots j give lane_id = how = track_len = -1.
 * 9. Coasted (frame, lane)s (sqair_set_observed) need no case of their own.
 * The memory and the counters are read, updated and written by the one workgroup of the lane, in place: a replayed graph leaves the
 * bits of eager calls, and two passes of three frames leave the bits of one pass of six.  A reset of a lane is the caller's: it frees
 * the entries (trk_id = -1) and keeps next_id, so an id is never reused within a lane.
 * lane_id is required, how and track_len are optional.  Pointers are remembered by the handle and frozen into captured graphs.  NULL
 * id: off.  Refused (return -1, text in sqair_last_error, before any HIP call): no estimate set (sqair_set_estimate); an estimate
 * without box, presence, obj_id or best_row; trk_what given while the estimate binds no what; a T other than the estimate's, a B
 * other than the state's; M outside N..16; iou_min outside (0, 1]; reid_dist negative; reid_what not in (0, +inf]; max_age < 0; any
 * NaN among the scalars; a NULL trk_id, trk_word, trk_age, trk_len, trk_box, next_id, counts or lane_id; at pass time: a pass of
 * another T.  sqair_set_estimate switching the estimate off, to another T or to one without those fields, and sqair_set_state
 * switching the state off or to another B, switch the identity off.
 * sqair_set_score_ids(h, 1) makes k_lane_score read the identity's lane_id words where it reads the estimate's obj_id (the kernel
 * treats the id as a 32-bit word: only the pointer the launcher passes changes); refused unless both the score and the identity are
 * set; the identity or the score going off puts it back to 0.
 * Out of scope: carrying lane_id into the object lists of lane tracks and lane forecasts; optimal (Hungarian) assignment (here: step 2
 * as keep + optimal is sqair_set_lane_match's, below; step 4 stays as it is); a motion model for the unseen track (not in this
 * kernel as it stands: sqair_set_motion, the motion paragraph below, is that opt-in); identities across lanes; training passes. */
#define SQAIR_IDENT_MAX_TRACKS 16
#define SQAIR_IDENT_COUNTS 8
typedef struct SqairLaneIdentity {
  float iou_min;        /* in (0, 1]: the position gate of the link */
  float reid_dist;      /* >= 0, pixels per frame: how far a centre may have moved per frame unseen; 0 = re-identification off */
  float reid_what;      /* in (0, +inf]: largest mean squared difference of what; +inf = rank by it, gate nothing */
  int32_t M;            /* track entries per lane, N..16 */
  int32_t max_age;      /* >= 0: frames a track may go unseen before it ends */
  /* memory, in/out, persists across passes; the caller starts with trk_id = -1, everything else 0 */
  int32_t* trk_id;      /* [B,M]  -1 = free */
  int32_t* trk_word;    /* [B,M]  the obj_id WORD last seen on the track */
  int32_t* trk_age;     /* [B,M]  frames since it was last seen */
  int32_t* trk_len;     /* [B,M]  frames it was seen in */
  float*   trk_box;     /* [B,M,4] its last box, the estimate's words */
  float*   trk_what;    /* [B,M,n_what] its last what, or NULL: no appearance, step 4 ranks by distance */
  int32_t* next_id;     /* [B]    the next fresh id of the lane */
  int64_t* counts;      /* [B,8]  frames, frames_invalid, objects, kept, bridged, reidentified, born, ended */
  /* per frame, out */
  int32_t* lane_id;     /* [T,B,N] required; -1 where slot j is absent */
  int32_t* how;         /* [T,B,N] 0 born, 1 kept (same obj_id word), 2 bridged (another word), 3 re-identified; -1 absent */
  int32_t* track_len;   /* [T,B,N] */
} SqairLaneIdentity;
int sqair_set_identity(SqairHandle* h, const SqairLaneIdentity* id /* NULL: off */, int T, int B);
/* Kernel-level check of the identity (tests): the kernel above on caller buffers, no state and no pass, with the handle's N and
 * n_what.  box [T,B,N,4], presence, obj_id [T,B,N], what [T,B,N,n_what] (or NULL) and best_row [T,B] stand for the estimate's outputs.
 * Refused (return -1, before any HIP call): a NULL box / presence / obj_id / best_row / id, T or B out of range, id->trk_what without
 * what, what sqair_set_identity refuses for id. */
int sqair_lane_identity_test(SqairHandle* h, const float* box, const float* presence, const float* obj_id, const float* what /* or NULL */,
                             const int32_t* best_row, int T, int B, const SqairLaneIdentity* id, void* stream);
int sqair_set_score_ids(SqairHandle* h, int lane_ids /* 0: the estimate's obj_id (default); 1: the identity's lane_id */);

/* ---- lane motion: a constant-velocity filter per track, inside the identity's kernel (the motion paragraph) ---------------------
 * The identity's position link compares a slot with the track's LAST box and its re-identification searches a disc that grows around
 * the last position: an object that moves more than about half its size per frame is born again every frame, and one that moves
 * while unseen returns outside the disc.  With a motion set, the identity's kernel node is REPLACED by a motion instantiation of the
 * same function (k_lane_identity_motion, or k_lane_identity_motion_opt under sqair_set_lane_match's identity = 1): the same node
 * count, the same place in the pass, one workgroup per lane.  With it off nothing changes and nothing more is launched: k_lane_identity
 * is the code it was, and every output, blob and accumulator is unchanged bit for bit.  Needs an identity (sqair_set_identity).
 * The state, per lane b, entry e < M and axis a in {y, x} of the box CENTRE: five fp32 words trk_kf[b,e,a,0..5) = (p, v, Ppp, Ppv,
 * Pvv) -- position, velocity in pixels per frame, and their covariance.  It is loaded into LDS with the rest of the table and
 * written back at the end of the pass.  The sizes h, w are not filtered: trk_box holds the last seen ones, as before.  Free entries
 * hold whatever they last held and are never read.  The caller starts with zeros.  The scalars: q > 0, the white-acceleration
 * variance; r > 0, the measurement variance in px^2; v0_var > 0, the velocity variance of a newborn track; gate > 0, in sigmas.
 * A non-finite lane (best_row[t,b] == -1) is untouched, as in point 0: no predict step, exactly as there is no ageing; its velocity
 * and nis are 0.  Per finite frame, the identity's points in their order, with these changes:
 * P. Predict, before point 1, one thread per (entry, axis) of every live entry: p += v; Ppp' = Ppp + 2 Ppv + Pvv + q/4; Ppv' = Ppv +
 *    Pvv + q/2; Pvv' = Pvv + q; S = Ppp' + r.  The entry's PREDICTED BOX is (p_y - h/2, p_x - w/2, h, w), h and w from trk_box.
 * 1. The IoU table uses the predicted box where it used trk_box[e].
 * 4. Tables: for every live e and present j, dy, dx = the slot's centre (fmaf(0.5, h, y), fmaf(0.5, w, x)) minus (p_y, p_x), and
 *    d2 = dy dy / S_y + dx dx / S_x.  Eligibility becomes d2 <= gate * gate (a NaN never passes): this replaces dc2 <= r * r, and
 *    reid_dist > 0 remains only the on/off switch of re-identification.  With trk_what the dw <= reid_what gate and the ranking by
 *    dw stay; without it the ranking key is d2, ties to the smallest e.  Still thread 0's walk, greedy in j.
 * Points 2, 3, 5, 6, 7 and 8 are untouched, including trk_box taking the slot's words.
 * U. Update, after the walk, one thread per (slot, axis).  For a slot linked to entry e by point 2 or 4, z its centre coordinate:
 *    y = z - p; k0 = Ppp'/S; k1 = Ppv'/S; p += k0 y; v += k1 y; Ppp = (1 - k0) Ppp'; Ppv = (1 - k0) Ppv'; Pvv = Pvv' - k1 Ppv'.
 *    For a slot born in point 6: (p, v, Ppp, Ppv, Pvv) = (z, 0, r, 0, v0_var), no predict in its birth frame.  Entries neither
 *    linked nor born keep the predicted state: an unseen track coasts at its velocity and its covariance grows, so the gate widens
 *    by itself.
 * Outputs per frame: velocity[t,b,j,0..2) = the posterior (v_y, v_x) of the slot's track, 0 for an absent slot, a non-finite lane
 * and a newborn; nis[t,b,j] (optional) = the d2 of the pair the slot was linked through, 0 for born or absent slots.
 * All arithmetic is fp32, every array in LDS, one code path for eager, captured and chunked runs: a replayed graph leaves the bits
 * of eager calls, two passes of six frames leave the bits of one pass of twelve.  A reset of a lane frees its entries as before;
 * nothing more is needed, a free entry's state is never read.
 * NULL m: off.  Refused (return -1, text in sqair_last_error, before any HIP call): no identity set (sqair_set_identity); a T other
 * than the estimate's, a B other than the state's; any of q, r, v0_var, gate not finite and positive; a NULL trk_kf or velocity.
 * The identity going off (sqair_set_identity(NULL), or the estimate or the state taking it along) switches the motion off.
 * Out of scope: filtering h, w; the particles' spread as r; lane_id and velocity in the object lists of lane tracks and lane
 * forecasts; training passes; identities across lanes. */
typedef struct SqairLaneMotion {
  float q, r, v0_var, gate;
  float* trk_kf;     /* [B,M,2,5] in/out, persists; caller starts with zeros */
  float* velocity;   /* [T,B,N,2] required */
  float* nis;        /* [T,B,N]   optional */
} SqairLaneMotion;
int sqair_set_motion(SqairHandle* h, const SqairLaneMotion* m /* NULL: off */, int T, int B);
/* Kernel-level check of the motion (tests): sqair_lane_identity_test with the motion instantiation on caller buffers.  NULL m: exactly
 * sqair_lane_identity_test.  Refused (return -1, before any HIP call): what that entry refuses, what sqair_set_motion refuses for m. */
int sqair_lane_identity_motion_test(SqairHandle* h, const float* box, const float* presence, const float* obj_id, const float* what,
                                    const int32_t* best_row, int T, int B, const SqairLaneIdentity* id, const SqairLaneMotion* m, void* stream);

/* ---- the track log: trajectories per lane_id, smoothed on the device (the track log paragraph) ----------------------------------
 * The identity and the motion answer for the current frame.  "Where was every object of the lane over the last frames" needs the
 * frames joined by lane_id, tracks that ended or are unseen included, and a gap filled by the motion model instead of left as a hole.
 * With a track log set, every following inference pass with a carried state, an estimate and an identity runs one more kernel,
 * k_lane_tracklog, one workgroup per lane over the pass's frames in order: directly after the identity's node, BEFORE k_lane_score if
 * on and BEFORE the SMC resampler.  A pass with the log on has exactly one kernel node more; with it off nothing is launched and every
 * other output, blob and accumulator is unchanged bit for bit.  Training passes, and a capture's eager pre-pass without effects, never
 * run it.  It reads only the identity's own output buffers lane_id and track_len and the estimate's box and best_row.
 * A. The log, per lane b, persistent on the device; L in 1..4096 records.  count [B] int64, the frames ever logged for the lane,
 *    invalid ones included, read and advanced on the device; the caller starts it at 0 (and the other fields at 0).  Frame t of a pass
 *    of T frames takes record (count[b] + t) mod L; after the pass count[b] += T.  A record holds
 *      log_valid [B,L] int32: 0 for a non-finite lane (best_row[t,b] == -1), else 1;
 *      log_id [B,L,N] int32: the word lane_id[t,b,j] as it stands: -1 where slot j is absent;
 *      log_len [B,L,N] int32: the word track_len[t,b,j] as it stands;
 *      log_box [B,L,N,4]: the estimate's four 32-bit words box[t,b,j], copied as they are.
 *    Every word of the record is written, whether the frame is valid or not: stale words are never read, and wrap-around needs no
 *    case of its own.  The ids of a record with log_valid == 0 are never looked at.  Words are copied, nothing is computed: a
 *    replayed graph leaves the bytes of eager calls, two passes of five and seven frames leave the bytes of one pass of twelve.
 * sqair_lane_tracklog_smooth, a stand-alone capturable call (one launch of k_lane_tracklog_smooth, one workgroup per lane), turns the
 * last `lag` records into trajectories.  It registers nothing, no pass runs it, it writes only its outputs and `work`: it may
 * interleave with passes.  C in 1..64 track columns; q, r, v0_var as in the motion paragraph.  For lane b:
 * 1. Window.  Frames f = 0..lag-1, oldest to newest: the absolute frame number is g = count[b] - lag + f, frame_index[f,b] = g, and
 *    its record is g mod L; g < 0 is "no record", frame_index = -1.  A frame COUNTS when it has a record with log_valid != 0.
 * 2. Columns.  The distinct ids >= 0 in the records of the frames that count; n_tracks[b] is their number.  The C largest are kept
 *    -- the newest ids: a tracker's caller wants the live tracks -- and listed ascending in track_id[b,0..C), padded with -1.  For a
 *    column, f0 and f1 are the first and the last frame that counts and holds its id (in a slot j, the smallest such j), and
 *    len0[b,c] is the log_len word of that slot at f0 (1: the track was born inside the window); -1 for a padding column.
 * 3. Forward filter, one thread per (column, axis a in {y, x} of the box CENTRE), the motion paragraph's P and U, the same
 *    statements in the same order (one device function each, shared with k_lane_identity_motion).  z = fmaf(0.5, size, origin) of
 *    the slot's box words, size = h or w.  At f0 the state starts as a newborn's, whatever len0 is: (p, v, Ppp, Ppv, Pvv) =
 *    (z, 0, r, 0, v0_var), state 1.  For f0 < f <= f1: a frame that counts does P; if the id is in the record it then does U with
 *    that slot's z (state 1, seen), otherwise the predicted state stands (state 2, a gap).  A frame inside the span that does not
 *    count does not step, exactly as the identity neither ages nor predicts there (state 3).  Outside the span the state is 0.
 * 4. Backward pass (Rauch-Tung-Striebel) over the STEPPED frames (state 1 or 2) in descending order; consecutive stepped frames
 *    are exactly one P apart.  At f1 the smoothed state is the filtered one.  For a stepped frame with filtered (p, v, a, b, c)
 *    and the smoothed (ps+, vs+, as+, bs+, cs+) of the next stepped frame, in fp32 and in this order:
 *      pm = p + v; am = ((a + 2 b) + c) + q/4; bm = (b + c) + q/2; cm = c + q             (P's statements)
 *      det = fmaf(am, cm, -(bm bm)); m00 = a + b; m10 = b + c
 *      g00 = fmaf(m00, cm, -(b bm)) / det; g01 = fmaf(b, am, -(m00 bm)) / det
 *      g10 = fmaf(m10, cm, -(c bm)) / det; g11 = fmaf(c, am, -(m10 bm)) / det             (G = P F^T (P-)^-1, F = [[1,1],[0,1]])
 *      dp = ps+ - pm; dv = vs+ - v; da = as+ - am; db = bs+ - bm; dc = cs+ - cm
 *      ps = fmaf(g01, dv, fmaf(g00, dp, p)); vs = fmaf(g11, dv, fmaf(g10, dp, v))          (x_s = x + G (x_s+ - x-))
 *      e00 = fmaf(g01, db, g00 da); e01 = fmaf(g01, dc, g00 db); e10 = fmaf(g11, db, g10 da); e11 = fmaf(g11, dc, g10 db)
 *      as = fmaf(e01, g01, fmaf(e00, g00, a)); bs = fmaf(e01, g11, fmaf(e00, g10, b)); cs = fmaf(e11, g11, fmaf(e10, g10, c))
 *    (P_s = P + G (P_s+ - P-) G^T).  The prediction is recomputed from the filtered state: only that is stored.
 * 5. Outputs: state [lag,B,C] int32; filt and smooth [lag,B,C,2,5] = (p, v, Ppp, Ppv, Pvv) per axis, 0 where the state is 0 or 3;
 *    size [lag,B,C,2] = the (h, w) words of the slot at state 1, the last seen ones at state 2, else 0: sizes are not filtered, as
 *    in the identity's predicted box.  All arithmetic is fp32, every sum in one fixed order, no decision depends on a threshold: the
 *    same bits come out of every replay, and with the same scalars filt's v at a seen frame after f0 of a column with len0 == 1 has
 *    the bits of the motion's velocity for that slot.
 * `work`: B * sqair_lane_tracklog_work_bytes(lag, C, N) bytes of the caller's, any content: the slot of every (frame, column); the
 * filtered states live in filt.  At the limits neither fits LDS.
 * Pointers are remembered by the handle and frozen into captured graphs.  NULL log: off.  sqair_set_tracklog is refused (return -1,
 * text in sqair_last_error, before any HIP call) with no identity set (sqair_set_identity); for an identity without track_len bound;
 * for a T other than the estimate's or a B other than the state's; for L outside 1..4096; for a NULL count, log_valid, log_id, log_len
 * or log_box.  The identity going off (sqair_set_identity(NULL), or the estimate or the state taking it along) switches the log off,
 * and so does sqair_set_identity registering an identity without track_len.
 * Out of scope: filtering h, w; lane_id inside the object lists of lane tracks and lane forecasts; scoring the log against truth
 * here (that is sqair_lane_tracklog_score's, next); training passes; identities across lanes. */
#define SQAIR_TRACKLOG_MAX_FRAMES 4096
#define SQAIR_TRACKLOG_MAX_TRACKS 64
typedef struct SqairLaneTrackLog {
  int32_t L;            /* records per lane, 1..4096 */
  /* the log, in/out, persists across passes; the caller starts with zeros */
  int64_t* count;       /* [B]       frames ever logged for the lane */
  int32_t* log_valid;   /* [B,L] */
  int32_t* log_id;      /* [B,L,N] */
  int32_t* log_len;     /* [B,L,N] */
  float*   log_box;     /* [B,L,N,4] */
} SqairLaneTrackLog;
int sqair_set_tracklog(SqairHandle* h, const SqairLaneTrackLog* log /* NULL: off */, int T, int B);
/* Kernel-level check of the append (tests): k_lane_tracklog on caller buffers, no state and no pass, with the handle's N.  lane_id,
 * track_len [T,B,N], best_row [T,B] and box [T,B,N,4] stand for the producers' outputs.  Refused (return -1, before any HIP call): a
 * NULL lane_id / track_len / best_row / box / log, T or B out of range, what sqair_set_tracklog refuses for log. */
int sqair_lane_tracklog_test(SqairHandle* h, const int32_t* lane_id, const int32_t* track_len, const int32_t* best_row, const float* box,
                             int T, int B, const SqairLaneTrackLog* log, void* stream);
/* The solve (points 1 to 5).  The handle gives the error text only.  Every output is required.  Refused (return -1, before any HIP
 * call): a NULL log, out or work, a NULL output; lag outside 1..L; C outside 1..64; N outside 1..16; B < 1; any of q, r, v0_var not
 * finite and positive; what sqair_set_tracklog refuses for log. */
typedef struct SqairTrackLogOut {
  int32_t* track_id;     /* [B,C]   ascending, -1 = padding */
  int32_t* n_tracks;     /* [B]     the distinct ids of the window, kept or not */
  int32_t* len0;         /* [B,C] */
  int64_t* frame_index;  /* [lag,B] the absolute frame number, -1 = no record */
  int32_t* state;        /* [lag,B,C] 0 outside the span, 1 seen, 2 gap, 3 a frame that does not count inside the span */
  float*   size;         /* [lag,B,C,2] */
  float*   filt;         /* [lag,B,C,2,5] */
  float*   smooth;       /* [lag,B,C,2,5] */
} SqairTrackLogOut;
int64_t sqair_lane_tracklog_work_bytes(int lag, int C, int N);   /* per lane; 0 for arguments the solve refuses */
int sqair_lane_tracklog_smooth(SqairHandle* h, const SqairLaneTrackLog* log, int lag, int C, int N, int B, float q, float r, float v0_var,
                               const SqairTrackLogOut* out, void* work, void* stream);
/* The log is scored against truth by sqair_lane_tracklog_score, next. */

/* ---- track log scoring: the solve's trajectories against ground-truth boxes (the track log scoring paragraph) -----------------------
 * The track log answers "where was every lane_id over the last frames", filtered causally and smoothed, gaps filled by the motion
 * model.  sqair_lane_tracklog_score says what that is worth on a stream with truth: does gap filling turn misses into hits or into
 * false positives, does smoothing move the boxes towards the truth, is sigma honest, do the trajectories keep their identity.  It is a
 * stand-alone, capturable call, one launch of k_lane_tracklog_score, one workgroup of four wavefronts per lane: it registers nothing,
 * no pass runs it, and it writes only `score`.  It is a pure function of its inputs -- nothing of `score` is read, there are no in/out
 * accumulators: the windows of successive calls overlap, so summing over calls is the caller's business.  The handle gives the error
 * text only.
 * Inputs.  `table` (read-only) is what sqair_lane_tracklog_smooth wrote for the same lag, C and B: track_id, frame_index, state, size,
 * filt and smooth are read.  `log` gives L, count and log_valid, so that a non-finite frame is told from an empty one.  `truth` is in
 * WINDOW ORDER, oldest to newest, as for sqair_lane_traj_score -- the caller brings the truth of the table's frames --: G in 1..16
 * slots per lane, truth_box [lag,B,G,4] fp32 (y, x, h, w) in pixels, truth_present [lag,B,G] and truth_valid [lag,B] int32 (nonzero =
 * set); truth identity IS the slot g, as in sqair_set_score.  score->iou_min in (0, 1].  match: 0 greedy, 1 optimal (point 3).
 * 1. Views.  Four views v = 0..3 of the one table, src = v & 1 (0: filt, 1: smooth), fill = v >> 1.  Column c is PRESENT in view v at
 *    frame f when state[f,b,c] == 1, or when fill is set and state[f,b,c] == 2.  Its box is (fmaf(-0.5f, h, p_y), fmaf(-0.5f, w, p_x),
 *    h, w) with p the word 0 of src[f,b,c,axis,:] and (h, w) = size[f,b,c,:].  View 0 is what a causal tracker reported; view 3 is
 *    what the MOTChallenge rows of the log export.  Wavefront v owns view v; the views share nothing.
 * 2. Frames.  Frame f of lane b is SCORED when frame_index[f,b] >= 0, its record (frame_index mod L) has log_valid != 0, and
 *    truth_valid[f,b] != 0.  A frame with a record and truth but log_valid == 0 counts one frames_invalid and nothing else; every
 *    other frame changes nothing.  The per-frame outputs of a frame that is not scored are -1 (match) and 0 (match_iou).
 * 3. Per scored frame and view, frames in ascending order.  Candidates: present truth g (truth_present != 0) x present column c;
 *    holes are allowed on both sides.  IoU(g, c) is sq_box_iou, the estimate's device function, on the fp32 words.  The assignment is
 *    the score's own device function, unchanged -- sq_assign_keep_greedy (match == 0) or sq_assign_keep_optimal (match == 1; the
 *    per-frame matching paragraph) -- with N := C, col_id[c] = track_id[b,c] and keep_id[g] = last[v][g], the track_id truth g was
 *    last matched with in this view, -1 at the start of EVERY call.  Events, exactly as point 4 of the stream scoring paragraph
 *    defines them: tp = matched pairs, fn = present truths unmatched, fp = present columns unclaimed; for each matched g in index
 *    order with id = track_id[b,c]: idsw += [last[v][g] >= 0 and last[v][g] != id], then last[v][g] = id; match[v,f,b,g] = c (-1
 *    unmatched or absent), match_iou[v,f,b,g] = the pair's IoU (0 unmatched).
 * 4. For each matched pair (g, c), in fp32 and in this order, with (t_y, t_x, th, tw) the truth's words, p_y, p_x the view's centre
 *    words and Ppp_y, Ppp_x the words 2 of the view's src per axis:  ty = fmaf(0.5f, th, t_y); tx = fmaf(0.5f, tw, t_x); dy = ty - p_y;
 *    dx = tx - p_x; err = sqrtf(fmaf(dy, dy, dx * dx)).  When both Ppp_y > 0 and Ppp_x > 0 (a NaN or a non-positive variance is not
 *    counted): nees = dy * dy / Ppp_y + dx * dx / Ppp_x, and the pair counts in nees_n; its expectation is 2 for an honest sigma.  A
 *    pair whose column is at state 2 also counts in gap_tp, gap_err_sum and, when its nees counts, in gap_nees_sum and gap_nees_n; a
 *    present, unclaimed column at state 2 counts in gap_fp.  (Views 0 and 1 hold no column at state 2: their gap figures are 0.)
 * 5. IDF over the window, per view.  ov[g][c] (int32) = the number of scored frames in which g and c are candidates with IoU(g, c) >=
 *    iou_min -- all such pairs, no one-to-one: the overlap table of Ristani et al., point 3d of the IDF1 paragraph.  After the last
 *    frame sq_assign_optimal_i32(ov, C, G, C, .), the IDF1 solve's device function: idtp = the optimum, idfn = (present truths over
 *    the scored frames) - idtp, idfp = (present columns over the scored frames) - idtp, assign[v,b,g] = the column assigned to g
 *    when their overlap is positive, else -1 (optimal assignments tie, the figures do not).  The weights are <= lag <= 4096, far
 *    inside the solver's exact range.
 * 6. Outputs.  counts [B,4,14] int64 per (lane, view) = frames (scored), frames_invalid, truth, tp, fn, fp, idsw, gap_tp, gap_fp,
 *    nees_n, gap_nees_n, idtp, idfn, idfp.  sums [B,4,5] fp64 = iou_sum, err_sum, nees_sum, gap_err_sum, gap_nees_sum: each fp32 value
 *    converted to fp64 and added by one thread, g in index order, frames in order -- no float atomics, so a replayed graph gives the
 *    bits of an eager call.  Both are required and every word of them is written; assign [4,B,G], match and match_iou [4,lag,B,G] are
 *    optional.
 * 7. Refused (return -1, text in sqair_last_error, before any HIP call): a NULL log, table, truth or score; what sqair_set_tracklog
 *    refuses for log; a NULL track_id, frame_index, state, size, filt or smooth of the table; a NULL truth_box, truth_present or
 *    truth_valid; a NULL counts or sums; lag outside 1..L; C outside 1..64; G outside 1..16; B < 1; iou_min NaN or outside (0, 1];
 *    match other than 0 or 1.
 * Out of scope: sums that persist over windows; HOTA of the log; scoring per particle row; filtering h, w; truth identities other
 * than the slot. */
#define SQAIR_TRACKLOG_SCORE_VIEWS 4
#define SQAIR_TRACKLOG_SCORE_COUNTS 14
#define SQAIR_TRACKLOG_SCORE_SUMS 5
typedef struct SqairTrackLogTruth {
  int32_t G;                      /* truth slots per lane, 1..16 */
  const float* truth_box;         /* [lag,B,G,4] window order */
  const int32_t* truth_present;   /* [lag,B,G] */
  const int32_t* truth_valid;     /* [lag,B] */
} SqairTrackLogTruth;
typedef struct SqairTrackLogScore {
  float iou_min;                  /* in (0, 1] */
  int64_t* counts;                /* [B,4,14] */
  double* sums;                   /* [B,4,5] */
  int32_t* assign;                /* [4,B,G]; optional */
  int32_t* match;                 /* [4,lag,B,G]; optional */
  float* match_iou;               /* [4,lag,B,G]; optional */
} SqairTrackLogScore;
int sqair_lane_tracklog_score(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table /* read-only */,
                              const SqairTrackLogTruth* truth, const SqairTrackLogScore* score,
                              int lag, int C, int B, int match /* 0 greedy, 1 optimal */, void* stream);

/* ---- motion calibration: fit q and r to the track log, without truth (the track log fit paragraph) --------------------------------
 * The motion filter, the solve and the scorer all stand on hand-set scalars q and r; the scorer says whether they fit only where
 * there is truth.  The filter's own innovations say it without: for a (q, r) the innovations y and their variances S of a track
 * define the likelihood -log p = 1/2 sum (ln 2 pi S + y y / S), its minimum over a grid of candidates is the maximum-likelihood fit,
 * and mean y y / S (the NIS) is 1 per axis for an honest filter.  sqair_lane_tracklog_fit forms the sums of that likelihood for every
 * candidate of a Q x R grid.  It is a stand-alone, capturable call, one launch of k_lane_tracklog_fit: it registers nothing, no pass
 * runs it, and it writes only its outputs -- counts, sums and innov; nothing of them is read.  The handle gives the error text only.
 * Inputs.  `table` and `work` (both read-only) are what sqair_lane_tracklog_smooth wrote for the same lag, C, N and B: of the table
 * only frame_index and state are read, of `work` the slot of every (frame, column); of `log`, L and log_box.  A frame's record is
 * frame_index mod L, as in the scorer.  No pass may have run between the solve and the fit: a pass moves the ring under the table.
 * The walk, per lane b, per candidate (iq, ir) with (q, r) = (fit->q[iq], fit->r[ir]), per column c and per axis a in {y, x}, frames in
 * ascending order, st = state[f,b,c]:
 * 1. st 0 or 3: nothing happens.
 * 2. The first st == 1: the state starts as a newborn's, (p, v, Ppp, Ppv, Pvv) = (z, 0, r, 0, v0_var), with z = fmaf(0.5, size,
 *    origin) of the slot's box words, exactly as in the solve's point 3; i = 0, gap = false.
 * 3. st == 2: P; gap = true.
 * 4. A later st == 1: S = P's return; y = z - p; nis = (y * y) / S in fp32; i += 1.  If i > burn, the term COUNTS when S > 0 and nis
 *    is finite: n += 1, nis_sum += (double)nis, lns_sum += log((double)S) -- the logarithm taken in fp64, so that no fp32 logf enters
 *    the definition --, and the same three into n_gap, gap_nis_sum, gap_lns_sum when gap is set; if i > burn and the term does not
 *    count, skipped += 1.  Then U; gap = false.  innov[f,b,c,a,:] = (y, S) for candidate (0, 0) at these frames, whatever burn is; 0
 *    everywhere else.
 * 5. The filter is sq_kf_predict and sq_kf_update, the motion paragraph's P and U: called, not restated.
 * Order of the sums.  A (candidate, column, axis) adds its terms in frame order in fp64; one thread then adds a candidate's 2 C
 * partial sums in (c, a) index order.  No float atomics: a replayed graph gives the bits of an eager call.  Every word of every
 * output is written.  counts [B,Q,R,3] int64 = n, n_gap, skipped; sums [B,Q,R,4] fp64 = nis_sum, lns_sum, gap_nis_sum, gap_lns_sum.
 * The candidate's negative log-likelihood is 1/2 (n ln 2 pi + lns_sum + nis_sum), formed by the caller.
 * Conditioning.  The fit conditions on the associations the log recorded: it does not re-link objects under a candidate's scalars.
 * Refused (return -1, text in sqair_last_error, before any HIP call): a NULL log, table, work or fit; what sqair_set_tracklog refuses
 * for log; a NULL frame_index or state of the table; a NULL counts or sums; lag outside 1..L; C outside 1..64; N outside 1..16; B < 1;
 * Q or R outside 1..16; burn < 0; v0_var or any read q[i] / r[i] not finite and positive.
 * Out of scope: fitting v0_var or gate; gradient or EM refinement inside a grid cell (call again with a finer grid); per-track or
 * per-lane scalars inside the identity kernel; re-linking under the candidate scalars; the particles' spread as r; filtering h, w;
 * sums that persist over windows; training passes. */
#define SQAIR_TRACKLOG_FIT_MAX_GRID 16
#define SQAIR_TRACKLOG_FIT_COUNTS 3      /* n, n_gap, skipped */
#define SQAIR_TRACKLOG_FIT_SUMS 4        /* nis_sum, lns_sum, gap_nis_sum, gap_lns_sum */
typedef struct SqairTrackLogFit {
  int32_t Q, R;          /* grid sizes, 1..16 each */
  int32_t burn;          /* >= 0: the first `burn` innovations of a column are not counted */
  float v0_var;          /* > 0, as in the motion paragraph */
  float q[16], r[16];    /* the first Q / R are read; each finite and > 0.  (The header parser takes a literal length only.) */
  int64_t* counts;       /* [B,Q,R,3] required */
  double*  sums;         /* [B,Q,R,4] required */
  float*   innov;        /* [lag,B,C,2,2] optional: (y, S) of candidate (0, 0) */
} SqairTrackLogFit;
int sqair_lane_tracklog_fit(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table /* read-only */,
                            const void* work /* read-only: as the solve left it */, const SqairTrackLogFit* fit,
                            int lag, int C, int N, int B, void* stream);

/* ---- track log stitching: join a track's fragments with hindsight (the track log stitching paragraph) --------------------------------
 * The identity kernel looks backwards only: it re-identifies an object with a track unseen for at most max_age frames, and its gate
 * is on position, because a newborn has no velocity yet.  So one object often sits in the solve's table as several columns with
 * disjoint spans, each smoothed on its own.  The log holds what a causal tracker never has: the later frames of the new fragment, and
 * so its velocity at its birth.  sqair_lane_tracklog_stitch links fragments by that hindsight and solves the joined columns again.  It
 * is a stand-alone, capturable call, one launch of k_lane_tracklog_stitch, one workgroup of 256 threads per lane: it registers nothing,
 * no pass runs it, it reads nothing of a previous call, and it writes only its outputs -- `stitched`, `work_out` and the link outputs;
 * nothing of them is read but what this launch wrote.  The handle gives the error text only.
 * Inputs (read-only).  `log`; `table` and `work` exactly as sqair_lane_tracklog_smooth left them for the same lag, C, N and B; q, r,
 * v0_var, the solve's.  No pass may have run between the solve and the stitch: a pass moves the ring under the table.  stitch->gate,
 * finite and > 0, in sigmas; stitch->max_gap in 0..lag.  `stitched` is a second SqairTrackLogOut of the same lag, C and B, `work_out`
 * a second `work` of the same size; both are outputs.  For lane b:
 * 1. Fragments.  The kept columns c with track_id[b,c] >= 0.  f0_c and f1_c are the first and the last frame with state[f,b,c] != 0;
 *    both are state 1 by the solve's construction.
 * 2. Candidates.  A link a -> b (a != b, both fragments) is a candidate when f1_a < f0_b; len0[b,cb] == 1 -- the successor was born at
 *    f0_b, inside the window, after the predecessor was last seen --; and gap <= max_gap, gap being the number of frames strictly
 *    between f1_a and f0_b that COUNT in the solve's sense (point 1 of the track log paragraph).
 * 3. Distance, per axis in {y, x}, in fp32 and in this order.  (pa, va, Aa, Ba, Ca) = filt[f1_a,b,a,axis,:] coasted with P
 *    (sq_kf_predict, called, not restated) once per frame that counts in (f1_a, f0_b], gap + 1 times: frames that do not count do not
 *    step, as in the solve.  (pb, vb, Ab, Bb, Cb) = smooth[f0_b,b,cb,axis,:], the successor's backward-informed birth state under
 *    its diffuse start prior.  The two rest on disjoint measurements, so their difference has covariance Pa + Pb:
 *      A = Aa + Ab; Bm = Ba + Bb; Cm = Ca + Cb; det = fmaf(A, Cm, -(Bm Bm)); dp = pb - pa; dv = vb - va
 *      num = fmaf(A dv, dv, fmaf(-2, Bm dv, Cm dp) dp); d2_axis = num / det          (= (Cm dp^2 - 2 Bm dp dv + A dv^2) / det)
 *    d2 = d2_y + d2_x, four degrees of freedom.  A candidate is ELIGIBLE when det_y > 0, det_x > 0 and d2 <= gate gate (the product
 *    formed in fp32).  A NaN never passes.
 * 4. Assignment over the C x C table in LDS (at most 16 KiB), rows = predecessors, columns = successors: weight 2^28 + q for an
 *    eligible pair, q = min(max(__float2int_rn((1 - d2 / (gate gate)) * 1048576.0f), 0), 2^20); -1 for every other pair.  Wave 0 calls
 *    sq_assign_optimal_i32, the IDF1 solve's device function.  64 pairs x 2^20 < 2^28: cardinality first, the smallest total d2 (in
 *    units of gate^2 2^-20) second; every weight is below 2^30, the solver's exact range.  Among equally optimal assignments the
 *    result is the solver's: deterministic, not restated as a rule.
 * 5. Chains.  A fragment has at most one successor and one predecessor and links go forward in time: they form chains of
 *    time-disjoint fragments.  A chain's root is its first fragment; it has the chain's smallest column and id.
 * 6. The stitched table, SqairTrackLogOut's layout with the same lag, C and B: one column per chain, in the order of the roots'
 *    columns -- track_id = the root's id, ascending, padded with -1 --; len0 the root's; n_tracks = the solve's minus the number of
 *    links; frame_index copied.  work_out[f,c'] = the `work` word of the chain's fragment whose span f0..f1 holds f (taken only inside
 *    0..N-1), -1 elsewhere.  On these columns, with f0 the root's and f1 the last fragment's, points 3 and 4 of the track log
 *    paragraph run as they stand -- ONE device function, sq_tracklog_walk, called by both kernels --: a bridged frame that counts is
 *    state 2 and is interpolated with the measurements of both sides, one that does not count is state 3; size, filt and smooth
 *    follow that paragraph's point 5.  The stitched table is by definition what the solve would have written had the identity kept
 *    one id: where it did, the bits are the solve's.
 * 7. Link outputs, every word written: link_next [B,C] int32, the successor's column in the SOLVE's table, -1 without one; link_d2
 *    [B,C] fp32, the link's d2, 0 without one; link_gap [B,C] int32, the link's gap, -1 without one; root [B,C] int32, the stitched
 *    column the solve's column went to, -1 for a padding column; n_links [B] int32.
 * Refused (return -1, text in sqair_last_error, before any HIP call): a NULL log, table, work, stitch, stitched or work_out; what
 * sqair_set_tracklog refuses for log; lag outside 1..L; C outside 1..64; N outside 1..16; B < 1; any of q, r, v0_var not finite and
 * positive; a NULL track_id, n_tracks, len0, frame_index, state, filt or smooth of the table; a NULL field of stitched; a NULL
 * link_next, link_d2, link_gap, root or n_links; gate not finite and positive; max_gap outside 0..lag; a field of stitched, or work_out,
 * sharing its pointer with a field of the table or with work.
 * Out of scope: re-linking inside a fragment; splitting a track; appearance in the distance (the log does not hold it); fitting on
 * the stitched table; links to tracks not among the C kept columns; a stated tie rule; stitching inside the pass or feeding links
 * back to the identity kernel; filtering h, w; training passes. */
typedef struct SqairTrackLogStitch {
  float gate;            /* finite, > 0: a link needs d2 <= gate^2 */
  int32_t max_gap;       /* 0..lag: the counting frames a link may bridge */
  int32_t* link_next;    /* [B,C] */
  float*   link_d2;      /* [B,C] */
  int32_t* link_gap;     /* [B,C] */
  int32_t* root;         /* [B,C] */
  int32_t* n_links;      /* [B] */
} SqairTrackLogStitch;
int sqair_lane_tracklog_stitch(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table /* read-only */,
                               const void* work /* read-only: as the solve left it */, int lag, int C, int N, int B, float q, float r,
                               float v0_var, const SqairTrackLogStitch* stitch, const SqairTrackLogOut* stitched, void* work_out,
                               void* stream);

/* ---- IDF1 scoring: does an identity stay on an object over its life -- global identity assignment, solved on the device ---------
 * The score's idsw counts the moments an identity changes on a greedy per-frame match; it cannot say for how long the wrong id then
 * stays, and gives no credit for an object re-identified under its old id.  The identity measures of Ristani et al. (IDF1, IDP, IDR)
 * and the trajectory statistics (mostly tracked / partly tracked / mostly lost, fragmentations) can: they need, per lane, how many
 * frames every truth identity overlapped every predicted identity, and a maximum-weight one-to-one assignment over that table.  With
 * an IDF set, every following inference pass with a carried state, an estimate and a score runs one more kernel, k_lane_idf, one
 * workgroup per lane looping over the pass's frames in order: after k_lane_score and BEFORE the SMC resampler.  A pass with the IDF on
 * has exactly one kernel node more; with it off nothing is launched and every other output, blob and accumulator is unchanged bit for
 * bit.  Training passes, and a capture's eager pre-pass without effects, never run it.  sqair_lane_idf_solve, a stand-alone capturable
 * call (one launch of k_lane_idf_solve, one wavefront per lane), solves the assignment when the caller reads the score or a clip ends.
 * Everything after the IoU threshold is integer arithmetic: graph replay, eager calls and split passes agree exactly.
 * 1. Units.  A CLIP of lane b runs from the start, or from the last close of lane b, to the next close.  Truth identity IS the slot g,
 *    as in the score.  Predicted identity is the 32-bit id WORD k_lane_score is handed for the same pass: the obj_id word, or lane_id
 *    when sqair_set_score_ids(h, 1) is in force.  The inputs are the score's own truth_box, truth_present, truth_valid, iou_min and G,
 *    and the score's per-frame output truth_match, which must be bound.
 * 2. Table, per lane, persistent on the device, updated in place by the lane's one workgroup, no atomics; P in 1..64 columns:
 *    col_id [B,P] the id word of a column, -1 = free (the other words of a free column are whatever they last held and are never
 *    read); overlap [B,G,P] frames in which truth g and column p overlapped; row_frames [B,G] frames truth g was present; col_frames
 *    [B,P] frames the column's id was present; extra_frames [B] object-frames without a column; matched [B,G] frames the score matched
 *    truth g; frag [B,G] fragmentations of truth g; trk_state [B,G] bit 0 = tracked at g's last present frame, bit 1 = ever tracked;
 *    frames [B] frames accumulated in the open clip.  All int32.  The caller starts with col_id = -1 and everything else 0.
 * 3. Per scored (frame, lane) -- truth_valid[t,b] != 0 and the estimate's lane finite (map_count != -1); every other frame touches
 *    nothing, exactly as in the score -- frames[b] += 1 and:
 *    a. Columns.  For the present lane objects j (presence != 0) in index order: the column whose col_id equals j's id word is j's; a
 *       non-negative word that is in no column takes the first free column (its col_frames and overlap start at 0).  An object is
 *       UNKEYED -- extra_frames += 1 -- when its word is negative, when no column is free, or when an earlier j of the same frame
 *       holds the same word (ids are distinct within a frame, so each cell has one writer: the later j counts as unkeyed).  A frame
 *       with at least one unkeyed object adds 1 to totals.overflow_ids, at once.
 *    b. col_frames[col(j)] += 1 for every keyed j.
 *    c. row_frames[g] += 1 for every present truth g (truth_present != 0).
 *    d. overlap[g, col(j)] += 1 for EVERY pair (present g, keyed j) with sq_box_iou(truth_box[t,b,g], box[t,b,j]) >= iou_min -- the
 *       score's device function on the same fp32 words; all pairs, not only the score's matches: that is the IDF1 definition.
 *    e. matched[g] += [truth_match[t,b,g] >= 0] for every present g.
 *    f. For every present g: if g is matched now, was ever tracked (bit 1) and was not tracked at its previous present frame (bit 0),
 *       frag[g] += 1; then bit 0 = matched now, bit 1 |= matched now.
 * 4. Solve, per lane.  IDTP = the maximum over one-to-one assignments of truth rows to columns of the sum of overlap[g, p];
 *    unassigned rows and columns are allowed (the dummy-node formulation of the paper), free columns count nothing.  IDFN = sum_g
 *    row_frames - IDTP, IDFP = sum_p col_frames (used columns) + extra_frames - IDTP.  A truth with row_frames > 0 is a trajectory;
 *    with m = matched and n = row_frames it is mostly tracked (MT) if 5 m >= 4 n, mostly lost (ML) if 5 m < n, partly tracked (PT)
 *    otherwise.  The clip's twelve figures, in the order of totals: clips (1 for a clip with frames > 0), frames, trajectories, idtp,
 *    idfn, idfp, mt, pt, ml, frag (sum_g frag), ids (columns used), overflow_ids (always 0 here: 3a has counted it in totals).
 *    assign[b,g] = the id word of the column assigned to truth g when their overlap is positive, else -1; optimal assignments tie,
 *    the figures do not.  The assignment is sq_assign_optimal_i32 (csrc/sqair_lane.h): shortest augmenting paths with integer
 *    potentials, rows inserted in index order, exact for weights below 2^30, which the frames of a clip never reach.
 * 5. Totals and close.  totals [B,12] int64, in/out, the caller zeroes them.  Without `close` the solve writes the open clip's figures
 *    to open [B,12] int64 and assign [B,G] (each optional) and changes nothing else.  For a lane with close[b] != 0 it also adds the
 *    figures to totals[b] and frees the table: col_id = -1 for every column, row_frames, matched, frag, trk_state, extra_frames and
 *    frames = 0; overlap and col_frames of a freed column stay as they are and are never read.
 * Pointers are remembered by the handle and frozen into captured graphs.  NULL idf: off.  sqair_set_idf is refused (return -1, text
 * in sqair_last_error, before any HIP call) with no score set (sqair_set_score); with a score that binds no truth_match; for a T other
 * than the estimate's or a B other than the state's; for P outside 1..64; for a NULL col_id, overlap, row_frames, col_frames,
 * extra_frames, matched, frag, trk_state, frames or totals.  The IDF goes off with the score: everything that switches the score off
 * switches it off, and so does sqair_set_score registering a score without truth_match or with another G.
 * Out of scope: optimal per-frame matching inside k_lane_score or k_lane_identity (the device function is shaped for it:
 * sqair_set_lane_match, below, is that change); truth
 * identities other than the slot; HOTA (sqair_set_hota, below); IDF1 per particle row, or for forecasts and lane tracks; identities across lanes; training
 * passes; more than 64 predicted ids per clip -- reported through overflow_ids, not solved. */
#define SQAIR_IDF_MAX_IDS 64
#define SQAIR_IDF_TOTALS 12
typedef struct SqairLaneIdf {
  int32_t P;                      /* id columns per lane, 1..64 */
  /* the table, in/out, persists across passes; the caller starts with col_id = -1, everything else 0 */
  int32_t* col_id;                /* [B,P]   the id word of the column, -1 = free */
  int32_t* overlap;               /* [B,G,P] */
  int32_t* row_frames;            /* [B,G] */
  int32_t* col_frames;            /* [B,P] */
  int32_t* extra_frames;          /* [B] */
  int32_t* matched;               /* [B,G] */
  int32_t* frag;                  /* [B,G] */
  int32_t* trk_state;             /* [B,G] */
  int32_t* frames;                /* [B] */
  int64_t* totals;                /* [B,12] in/out: clips, frames, trajectories, idtp, idfn, idfp, mt, pt, ml, frag, ids, overflow_ids */
} SqairLaneIdf;
int sqair_set_idf(SqairHandle* h, const SqairLaneIdf* idf /* NULL: off */, int T, int B);
/* Kernel-level check of the accumulation (tests): k_lane_idf on caller buffers, no state and no pass, with the handle's N and any G
 * in 1..16.  box [T,B,N,4], presence, ids [T,B,N] (32-bit words) and map_count [T,B] stand for the estimate's outputs, score for the
 * registered score: its truth_box, truth_present, truth_valid, iou_min, G and truth_match [T,B,G] are read, nothing of it is written.
 * Refused (return -1, before any HIP call): a NULL box / presence / ids / map_count / score / idf, T or B out of range, G or iou_min
 * out of range, a NULL truth_box, truth_present, truth_valid or truth_match, what sqair_set_idf refuses for idf. */
int sqair_lane_idf_test(SqairHandle* h, const float* box, const float* presence, const float* ids, const int32_t* map_count, int T, int B,
                        const SqairLaneScore* score, const SqairLaneIdf* idf, void* stream);
/* The solve (points 4 and 5): stand-alone and capturable -- nothing is registered on the handle and no pass runs it.  It takes the
 * caller's tensors, so the tests call the kernel through it as it stands.  The handle gives the error text only.  Refused (return -1, before any HIP call): a
 * NULL idf, G outside 1..16, B < 1, what sqair_set_idf refuses for idf. */
int sqair_lane_idf_solve(SqairHandle* h, const SqairLaneIdf* idf, int G, int B, const int32_t* close /* device [B] or NULL */,
                         int64_t* open /* [B,12] or NULL */, int32_t* assign /* [B,G] or NULL */, void* stream);

/* ---- HOTA scoring: detection, association and localisation in one figure -- a per-clip match log, a two-pass solve on the device ---
 * CLEAR-MOT (sqair_set_score) is dominated by detection, IDF1 (sqair_set_idf) by association.  HOTA (Luiten et al., IJCV 2020)
 * separates detection (DetA), association (AssA) and localisation (LocA) and combines them, HOTA_a = sqrt(DetA_a AssA_a), over nineteen
 * localisation thresholds a = 0.05 i.  It needs two passes over a clip: the per-frame matching maximises IoU x a global alignment score
 * between a truth identity and a predicted identity, and that score needs the whole clip.  So with a HOTA set, every following
 * inference pass with a carried state, an estimate and a score runs one more kernel, k_lane_hota, one workgroup per lane looping over
 * the pass's frames in order, which appends one record per scored frame to the lane's CLIP LOG: after k_lane_score (and after
 * k_lane_idf when that is on) and BEFORE the SMC resampler.  A pass with HOTA on has exactly one kernel node more; with it off nothing
 * is launched and every other output, blob and accumulator is unchanged bit for bit.  Training passes, and a capture's eager pre-pass
 * without effects, never run it.  sqair_lane_hota_solve, a stand-alone capturable call (one launch of k_lane_hota_solve, one workgroup
 * per lane), makes both passes over the log when the caller reads the score or a clip ends.  After the fp32 IoU everything is integer
 * arithmetic: graph replay, eager calls and split passes agree exactly.
 * 1. Units.  A clip, the truth identity (the slot g) and the predicted identity (the id word the score is handed) are exactly the
 *    IDF's points 1 and 3: scored frames are those with truth_valid != 0 and map_count != -1, every other frame touches nothing.  The
 *    columns follow the IDF's rule 3a in a column table of HOTA's own, col_id [B,P], P in 1..64, -1 = free: HOTA works with or without
 *    an IDF.  The score's iou_min and truth_match are NOT read: HOTA has its own thresholds and its own matching.
 * 2. Log, per lane, persistent on the device, written by the lane's one workgroup; L in 1..4096 records.  A scored frame takes the
 *    next record, number frames[b], and frames[b] += 1; with the log full (frames[b] == L) the frame adds 1 to dropped_frames[b] and
 *    touches nothing else -- no column either.  A record holds
 *      log_q   [B,L,G,N] int32  q = __float2int_rn(IoU * 1048576.0f), the IoU of sq_box_iou on the words the score reads in units of
 *                               2^-20, for a present truth g and a KEYED present object j; -1 for every other pair;
 *      log_col [B,L,N]   int32  the column of j; -1: j is absent, -2: j is present but unkeyed;
 *      log_row [B,L]     int32  bit g is set when truth g is present.
 *    Every word of a record in use was written when it was taken: stale log words are never read.  A frame with at least one unkeyed
 *    object adds 1 to totals_c.overflow_ids, at once.  All int32; the caller starts with col_id = -1, frames and dropped_frames 0.
 * 3. Solve, pass 1, over the lane's records in order.  Per record, over its pairs with q >= 0: R_g = sum_j q, C_j = sum_g q and
 *    n(g,j) = (q * 2^20) / (R_g + C_j - q) in int64, truncating, 0 when the denominator is 0 -- the pair's share of everything either
 *    of the two overlaps in the frame; pot[g, col(j)] += n.  row_frames[g] += 1 for each present g, col_frames[col(j)] += 1 for each
 *    keyed j, extra += 1 for each unkeyed j.  Then gas[g,p] = (pot * 2^20) / ((row_frames[g] + col_frames[p]) * 2^20 - pot), 0 when
 *    the denominator is 0: TrackEval's global_alignment_score in units of 2^-20.
 * 4. Solve, pass 2: ONE assignment per record, not one per threshold.  w[g,j] = (gas[g, col(j)] * q[g,j]) >> 15 for the pairs with
 *    q >= 0, -1 elsewhere: w <= 2^25, sixteen pairs stay below 2^30, the exact range of sq_assign_optimal_i32 (csrc/sqair_lane.h),
 *    which is called on the table as it stands.  Among equally optimal assignments the result is whatever that function returns:
 *    deterministic, not restated as a rule.  For each matched pair and each threshold i = 1..19 with A_i = ceil(i * 2^20 / 20) -- so
 *    that A_10 = 2^19 --: if q >= A_i then tp_i += 1, loc_i += q and mc_i[g, col(j)] += 1.  match [B,L,G] (optional) = the j matched
 *    with truth g in each record in use, or -1.
 * 5. Figures, per lane and threshold: fn_i = sum_g row_frames - tp_i, fp_i = sum_p col_frames + extra - tp_i, and in double, in a
 *    fixed order (one thread, the cells (g, p) in index order) over the cells with mc_i > 0: ass_i = sum mc^2 / (row_frames[g] +
 *    col_frames[p] - mc), assre_i = sum mc^2 / row_frames[g], asspr_i = sum mc^2 / col_frames[p].  The integers do not depend on the
 *    schedule (mc is kept with integer atomics in the caller's scratch `work`), the doubles are summed after them.
 * 6. Totals and close, as for the IDF.  totals_i [B,19,4] int64 = (tp, fn, fp, loc), totals_f [B,19,3] double = (ass, assre, asspr),
 *    totals_c [B,4] int64 = (clips, frames, dropped_frames, overflow_ids; clips is 1 for a clip with frames > 0, overflow_ids always 0
 *    in a clip's figures: 2 has counted it), in/out, the caller zeroes them.  Without `close` the solve writes the open clip's figures
 *    to open_i, open_f, open_c (each optional, shaped as the totals) and match and changes nothing else but `work`.  For a lane with
 *    close[b] != 0 it also adds them to the totals and frees the lane: col_id = -1 for every column, frames and dropped_frames = 0.
 *    The totals combine clips the way TrackEval combines sequences: counts add, and AssA = ass / tp is weighted by TP.  The ratios are
 *    the caller's: DetA = tp / (tp + fn + fp), DetRe = tp / (tp + fn), DetPr = tp / (tp + fp), AssA = ass / tp, AssRe = assre / tp,
 *    AssPr = asspr / tp, LocA = loc / (2^20 tp), HOTA_a = sqrt(DetA AssA), and HOTA their mean over the nineteen thresholds.
 * Pointers are remembered by the handle and frozen into captured graphs.  NULL hota: off.  sqair_set_hota is refused (return -1, text
 * in sqair_last_error, before any HIP call) with no score set (sqair_set_score); for a T other than the estimate's or a B other than
 * the state's; for P outside 1..64; for L outside 1..4096; for a NULL col_id, log_q, log_col, log_row, frames, dropped_frames, work,
 * totals_i, totals_f or totals_c.  HOTA goes off with the score: everything that switches the score off switches it off, and so does
 * sqair_set_score registering a score with another G.
 * Out of scope: a tie rule among optimal assignments; HOTA per particle row, or for forecasts and lane tracks; truth identities other
 * than the slot; clips longer than L frames -- reported through dropped_frames, not scored; training passes. */
#define SQAIR_HOTA_ALPHAS 19
#define SQAIR_HOTA_MAX_IDS 64
#define SQAIR_HOTA_MAX_FRAMES 4096
typedef struct SqairLaneHota {
  int32_t P;                      /* id columns per lane, 1..64 */
  int32_t L;                      /* log records per lane, 1..4096 */
  /* the log, in/out, persists across passes; the caller starts with col_id = -1, frames and dropped_frames 0 */
  int32_t* col_id;                /* [B,P]     the id word of the column, -1 = free */
  int32_t* log_q;                 /* [B,L,G,N] */
  int32_t* log_col;               /* [B,L,N] */
  int32_t* log_row;               /* [B,L] */
  int32_t* frames;                /* [B] records in use */
  int32_t* dropped_frames;        /* [B] scored frames of the open clip that found the log full */
  int32_t* work;                  /* [B,G,P,20] the solve's scratch (the pair histogram); any content */
  int64_t* totals_i;              /* [B,19,4] in/out: tp, fn, fp, loc */
  double* totals_f;               /* [B,19,3] in/out: ass, assre, asspr */
  int64_t* totals_c;              /* [B,4] in/out: clips, frames, dropped_frames, overflow_ids */
} SqairLaneHota;
int sqair_set_hota(SqairHandle* h, const SqairLaneHota* hota /* NULL: off */, int T, int B);
/* Kernel-level check of the append (tests): k_lane_hota on caller buffers, no state and no pass, with the handle's N and any G in
 * 1..16.  box [T,B,N,4], presence, ids [T,B,N] (32-bit words) and map_count [T,B] stand for the estimate's outputs, score for the
 * registered score: its truth_box, truth_present, truth_valid and G are read, nothing of it is written.  Refused (return -1, before any
 * HIP call): a NULL box / presence / ids / map_count / score / hota, T or B out of range, G out of range, a NULL truth_box,
 * truth_present or truth_valid, what sqair_set_hota refuses for hota. */
int sqair_lane_hota_test(SqairHandle* h, const float* box, const float* presence, const float* ids, const int32_t* map_count, int T, int B,
                         const SqairLaneScore* score, const SqairLaneHota* hota, void* stream);
/* The solve (points 3 to 6): stand-alone and capturable -- nothing is registered on the handle and no pass runs it.  It takes the
 * caller's tensors, so the tests call the kernel through it as it stands.  The handle gives the error text only.  Refused (return -1,
 * before any HIP call): a NULL hota, G outside 1..16, N outside 1..16, B < 1, what sqair_set_hota refuses for hota. */
int sqair_lane_hota_solve(SqairHandle* h, const SqairLaneHota* hota, int G, int N, int B, const int32_t* close /* device [B] or NULL */,
                          int64_t* open_i /* [B,19,4] or NULL */, double* open_f /* [B,19,3] or NULL */, int64_t* open_c /* [B,4] or NULL */,
                          int32_t* match /* [B,L,G] or NULL */, void* stream);

/* ---- per-frame matching: keep + optimal where the lane block matches keep + greedy --------------------------------------------
 * The lane block makes three per-frame correspondences, each by keep + greedy: truth x lane object in the stream score (its points 2
 * and 3), track entry x lane object in the lane identities (their step 2), truth x lane object at the anchor of the trajectory score
 * (its point 1).  Greedy is not what CLEAR-MOT defines: it keeps the still-valid correspondences of the last frame and solves the
 * rest as an assignment problem.  With iou_min = 0.5 and the IoU table [[0.60, 0.54], [0.54, 0.08]] greedy takes (0, 0) and leaves
 * truth 1 with nothing eligible -- tp 1, fn 1, fp 1 where two pairs exist.  sqair_set_lane_match selects, for each of the three, which
 * of the two a launch uses; this paragraph is the one definition of the optimal mode.
 * 1. Values.  score, identity, traj_link: 0 = keep + greedy (the default: every output, blob, accumulator and graph node count is what
 *    it is without this call), 1 = keep + optimal.  score selects the mode of the stream score's kernel, identity that of step 2 of the
 *    identity's kernel (re-identification, births and ageing are untouched), traj_link that of the link of sqair_lane_traj_score.
 * 2. Keep.  Exactly the greedy mode's keep (the score's point 2), unchanged in meaning: rows in index order, the first unclaimed
 *    eligible column carrying the remembered id word.  A kept pair is never given up, even where that costs a pair: that is
 *    CLEAR-MOT's rule, and it keeps idsw comparable between the modes.
 * 3. Rest: the objective.  Among the rows still unmatched and the columns still unclaimed, the one-to-one assignment of eligible
 *    pairs (IoU >= iou_min; a NaN never passes; an absent row or column has no eligible pair) that maximises first the NUMBER of
 *    pairs, then the sum of q(g, j) over the pairs.  q = __float2int_rn(IoU * 1048576.0f): the fp32 IoU the greedy mode compares, in
 *    units of 2^-20, rounded to nearest even.
 * 4. Weights.  The wavefront builds an int32 table in LDS: 2^25 + q for an eligible pair of an unmatched row and an unclaimed
 *    column, -1 for every other pair.  IoU <= 1 gives q <= 2^20, at most 16 pairs give a sum of q of at most 2^24 < 2^25: one pair
 *    more outweighs every sum of q.  Every weight stays below 2^30, the exact range of sq_assign_optimal_i32 (the IDF1 solve's device
 *    function, called on the table as it stands), and a pair of weight -1 is never taken.  The function is sq_assign_keep_optimal
 *    (csrc/sqair_lane.h), one wavefront's work where the greedy mode is one thread's walk.
 * 5. Ties.  As in the IDF1 solve, optimal assignments tie: among equally optimal ones the result is whatever sq_assign_optimal_i32
 *    returns.  That is deterministic -- the same bits eager, graph-replayed and in split passes -- and is not restated as a rule.
 * 6. What follows.  Everything after the assignment is the greedy mode's code on the new pairs: the score's events, last_id,
 *    match_iou, truth_match and accumulators; the identity's how, updates, re-identification, births and ageing; the trajectory
 *    score's link, link_iou, lane_counts and every per-frame figure read through the link.  The IDF table's matched and frag (and
 *    with them MT / PT / ML) read the score's truth_match and so follow the score's mode; its overlap table and IDTP do not depend
 *    on it.  tp of a frame in the optimal mode is never below the greedy mode's on the same memory.
 * 7. A plain setting of the handle: it needs no registration, survives sqair_set_estimate / _score / _identity / _state switching
 *    things on and off, and is read when a pass or a stand-alone call is issued -- a captured graph freezes it, as it freezes
 *    pointers.  The kernel-level entries sqair_lane_score_test, sqair_lane_identity_test and sqair_lane_idf_test honour it (the
 *    last reads only truth_match, whatever mode wrote it).  The node count of a pass does not depend on it.
 * Refused (return -1, text in sqair_last_error, before any HIP call): a NULL handle; a value other than 0 or 1 -- nothing is changed
 * then.  Not offered: a stated tie-break among optimal assignments; optimal re-identification (the identity's step 4); matching per
 * particle row; HOTA (sqair_set_hota, above); training passes. */
int sqair_set_lane_match(SqairHandle* h, int score, int identity, int traj_link);

/* ---- objective ---------------------------------------------------------------------------------
 * Fused IWAE / VIMCO reductions over [T,B,K] (reference: Model._build sqair/model.py:88-103,
 * targets.iwae / vimco_control_variate / vimco sqair/targets.py:38-75, make_target model.py:150-158,
 * ops.ess ops.py:52-59, _imp_weighted_mean model.py:202-205).
 *   log_w_t, disc_lp_t: [T,B*K]; scalars_out[16]:
 *     0 elbo_vae  1 elbo_iwae  2 vimco_target (already / T)  3 ess
 *   iw_means_in/out: optional n_means x [T,B*K] tensors -> n_means importance-weighted per-frame means; both may be NULL
 *     with n_means = 0 only.  disc_lp_t and each of log_weights .. scalars_out may be NULL; scalars_out[4..15] and
 *     iw_means_out[n_means..7] are not written.  k_particles = 1 gives NaN for the VIMCO signal and target, like the reference.
 * Refused (return -1, text in sqair_last_error, before any HIP call): n_means > 0 with iw_means_in NULL, with a NULL among its
 * first n_means pointers, or with iw_means_out NULL; T * B * k_particles above 2147483647 (the kernels index with int). */
int sqair_elbo(SqairHandle* h, const float* log_w_t, const float* disc_lp_t, int T, int B,
               float* log_weights /*[B,K]*/, float* elbo_iwae_per_example /*[B]*/,
               float* importance_weights /*[B,K]*/, float* vimco_signal /*[B,K]*/, float* scalars_out /*[16]*/,
               const float* const* iw_means_in, int n_means, float* iw_means_out, void* stream);

/* ---- per-kernel entry points (unit parity tests; same kernels sqair_forward launches) ----------- */
/* SpatialTransformer forward crop (reference: sqair/modules.py:170-218): img [B,H,W] shared by K
 * consecutive rows, where_logits [R,4] (R = B*K), optional mask [R,G*G]; out [R,G*G]. */
int sqair_st_crop(SqairHandle* h, const float* img, const float* where_logits, const float* mask,
                  float* out, int B, void* stream);
/* AIRDecoder canvas + Gaussian log-likelihood (reference: sqair/modules.py:435-467, seq.py:271-274):
 * glimpse [R,N,G*G], where [R,N,4], presence [R,N], img [B,H,W], mean_img [H,W];
 * canvas [R,H,W] (optional), data_ll [R]. */
int sqair_st_insert_loglik(SqairHandle* h, const float* glimpse, const float* where_logits,
                           const float* presence, const float* img, const float* mean_img,
                           float* canvas, float* data_ll, int B, void* stream);
/* y = act(x W + b) on the packed MFMA path, W [K,N] packed by the planner that packs the handle's layers (test helper; so
 * are the packs of the test helpers below): act 0 none, 1 elu, 2 tanh, 3 sigmoid, 4 softplus+0.01. */
int sqair_linear_test(SqairHandle* h, const float* x, const float* w, const float* b, float* y, int M,
                      int Kdim, int Ndim, int act, void* scratch, int64_t scratch_bytes, void* stream);
/* snt.GRU step through the two fused MFMA launches the forward pass uses:
 * x [M,Kx], hstate [M,n_hidden]; gru_flat = for g in (z,r,h): w_g [Kx,nh], u_g [nh,nh], b_g [nh]
 * (the order of the reference's GRU variables inside the flat parameter buffer). */
int sqair_gru_test(SqairHandle* h, const float* x, const float* hstate, const float* gru_flat, float* h_out,
                   int M, int Kx, void* scratch, int64_t scratch_bytes, void* stream);

/* snt.LSTM step (time_transition / prior_transition = LSTM; dm_sonnet 1.14 restated: gates (i, j, f, o) =
 * [x, h] w_gates + b_gates; c' = sigmoid(f + 1) c + sigmoid(i) tanh(j); h' = tanh(c') sigmoid(o)):
 * lstm_flat = w_gates [(Kx + nh), 4 nh] then b_gates [4 nh]; state_out [M, 2 nh] = [h' | c']. */
int sqair_lstm_test(SqairHandle* h, const float* x, const float* hstate, const float* cstate, const float* lstm_flat,
                    float* state_out, int M, int Kx, void* scratch, int64_t scratch_bytes, void* stream);
/* adjoint of the element-wise cell: gate pre-activations [M, 4 nh], c_prev, d h', d c' -> d gates, d c_prev */
int sqair_lstm_cell_bwd_test(SqairHandle* h, const float* gates, const float* c_prev, const float* d_h, const float* d_c,
                             float* d_gates, float* d_cprev, int M, void* stream);
/* Slot compaction of ONE frame on raw device buffers (test helpers; reference: _choose_latents sqair/sqair_modules.py:514-582,
 * compute_object_ids / select_present sqair/index.py:132-221) and its adjoint: the launches of the frame loop and of the backward
 * sweep with the handle's dimensions, R = B * k_particles rows, then a stream synchronise.
 * sqair_compact_test_layout: fills out[0:n] with the widths and columns of THIS build's buffers (the product and the wide library
 * lay the slot record out differently) and returns the number of entries it knows (20):
 *   0 record width W | 1 PRES | 2 ID | 3 WHERE | 4 WHAT | 5 LOGIT | 6 WHERE_LOC | 7 WHERE_SCALE | 8 WHAT_LOC | 9 WHAT_SCALE | 10 PROB |
 *   11 temporal state width | 12 prior state width | 13 floats of `flat` | 14, 15 offsets of seq.temporal_init / seq.prior_init
 *   in `flat` | 16 slots the build takes | 17 N | 18 n_what | 19 1 if the handle's dimensions have a specialised instantiation.
 *   Widths are the kernels' own (n_hidden rounded up to 128 / 256 / 512; an LSTM state is [hidden | cell]); `flat` is the
 *   parameter buffer in the kernels' own layout (sqair_debug_padded_count floats).
 * sqair_compact_test: rec_p / rec_d / rec_prev [R][N][W], temporal_p [R][N][11], prior_p [R][N][12], last_id_prev [R] -> rec_next,
 *   temporal_next, prior_next, last_id_next, src_out [R][N] (source slot 0..2N-1 of every merged slot) and whichever of the ten
 *   per-slot outputs and num_steps_per_sample `out` names, at frame index t of tensors shaped [T][R][N][..].  Honours the
 *   "specialised" option.
 * sqair_compact_bwd_test: src [R][N] as the forward wrote it (refused, -1, unless every row names N distinct slots of [0, 2N));
 *   d_rec_p / d_rec_d are accumulated into, d_temporal_p / d_prior_p [R][N][..] and d_new_temporal / d_new_prior [R][..] written. */
int sqair_compact_test_layout(const SqairHandle* h, int32_t* out, int n);
int sqair_compact_test(SqairHandle* h, const float* rec_p, const float* rec_d, const float* rec_prev, const float* temporal_p,
                       const float* prior_p, const float* last_id_prev, const float* flat, float* rec_next, float* temporal_next,
                       float* prior_next, float* last_id_next, int32_t* src_out, const SqairOutputs* out, int t, int B, void* stream);
int sqair_compact_bwd_test(SqairHandle* h, const int32_t* src, const float* d_rec_next, const float* d_temporal_next,
                           const float* d_prior_next, float* d_rec_p, float* d_rec_d, float* d_temporal_p, float* d_prior_p,
                           float* d_new_temporal, float* d_new_prior, int B, void* stream);

/* ---- adjoint (backward) building blocks of the training step (sqair_st_crop_bwd,
 * sqair_st_insert_ll_bwd, ...; the reference gets them from TF autodiff, sqair/model.py:160) ---------- */
/* d/d(where logits) [R,4] and optionally d/d(mask) [R,G*G] of the (masked) crop, given d/d(out) [R,G*G]. */
int sqair_st_crop_bwd(SqairHandle* h, const float* img, const float* where_logits, const float* mask,
                      const float* g_out, float* d_where_logits, float* d_mask, int B, void* stream);
/* Adjoint of sqair_st_insert_loglik for an upstream gradient g_data_ll [R]: d_glimpse [R,N,G*G],
 * d_where_logits [R,N,4], d_mean_img [H,W] (summed over rows; NULL: not reduced, the per-row contributions stay in
 * scratch as [R, H*W]); scratch >= R*H*W*4 bytes. */
int sqair_st_insert_loglik_bwd(SqairHandle* h, const float* glimpse, const float* where_logits,
                               const float* presence, const float* img, const float* mean_img,
                               const float* g_data_ll, float* d_glimpse, float* d_where_logits,
                               float* d_mean_img, void* scratch, int64_t scratch_bytes, int B, void* stream);
/* Gradient of the VIMCO target (already / T) w.r.t. the per-frame log weights and discrete log-probs [T,B*K],
 * from the importance weights and the learning signal sqair_elbo returned.
 * Refused (return -1, text in sqair_last_error, before any HIP call): T * B * k_particles above 2147483647 (the kernel indexes
 * with int). */
int sqair_elbo_bwd(SqairHandle* h, const float* importance_weights, const float* vimco_signal, int T, int B,
                   float* g_log_w_t, float* g_disc_lp_t, void* stream);
/* Decoder branch of sqair_backward on its own (unit-test entry: the same host function and kernels as the full pass).
 * Call after sqair_forward (with SqairOutputs.glimpse == NULL so the decoded glimpses stay in the workspace) and
 * sqair_elbo on the same inference workspace.  Writes the gradients of the VIMCO target w.r.t. dec.mean_img,
 * dec.l{0,1,2}.{w,b}, dec.output_scale into flat_grad (flat-parameter layout; other entries untouched) and, optionally,
 * the seed gradients on the merged latents d_rec [T, B'*N, 64] (record order: where 0:4, what 4:54).  Refuses (-1) padded
 * configurations, the wide build, frames that cannot be trained and H * W that is not a multiple of 4.  `scratch`:
 * sqair_backward_scratch_bytes (query it: the size is the entry's own business). */
int64_t sqair_backward_scratch_bytes(const SqairHandle* h, int T, int B);
int sqair_backward_decoder(SqairHandle* h, const float* flat_params, const void* packed, const float* obs,
                           const float* importance_weights, const float* vimco_signal, int T, int B,
                           void* workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes,
                           float* flat_grad, float* d_rec_out, void* stream);
/* Full backward pass (replaces TF autodiff of Model.make_target, sqair/model.py:150-168,
 * through SequentialAIR / SQAIRTimestep, sqair/seq.py:60-150, sqair/sqair_modules.py:388-582): gradient of the VIMCO
 * target / T w.r.t. EVERY trainable parameter, written to flat_grad (flat-parameter layout, overwritten).
 * Call order on one stream:  sqair_forward_train(train_workspace)  ->  sqair_elbo  ->  sqair_backward with the same
 * obs / noise / T / B / t_offset, the importance weights and learning signal sqair_elbo returned.  `scratch` holds the
 * gradient records and pre-activation gradient tapes (sqair_backward_bytes). */
int64_t sqair_backward_bytes(const SqairHandle* h, int T, int B);
int sqair_backward(SqairHandle* h, const float* flat_params, const void* packed, const float* obs, const float* noise,
                   const float* importance_weights, const float* vimco_signal, int T, int B, int t_offset,
                   void* train_workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes,
                   float* flat_grad, void* stream);

/* ---- training with a carried state (truncated BPTT over a stream) -------------------------------------------------------
 * A carried training chunk is T' frames of B lanes that start from a state blob (the blob of sqair_set_state) instead of the
 * trainable initial state.  Row r starts from
 *   blob row src_rows[r] when state_in is set and src_rows[r] >= 0 (identity without src_rows): held CONSTANT -- no gradient
 *     flows into it, as with the noise -- and its frame counter is the blob's;
 *   the trainable initial state otherwise (src_rows[r] = -1 or outside [-1, B*K), or state_in NULL), counter 0: gradient
 *     flows into seq.temporal_init(_c) / seq.prior_init(_c) as in sqair_backward.
 * The frames run exactly as a pass does; the categorical step prior's t is the row's counter plus the frame index.  The target
 * is the one of sqair_elbo on [T', B*K] unchanged: VIMCO over the chunk's own log weights and discrete log-probs, / T'.  Log
 * weights of earlier chunks are NOT part of it.  sqair_backward_carry returns d target / d theta with the imported rows held
 * constant.  After the forward, frame T''s state (records, cell states, ids, counters) goes to state_out, exactly as an
 * inference pass exports it, so that a video trained chunk by chunk carries identities and counters from chunk to chunk.
 * The backward reads neither the blob nor src_rows: the forward records in the training workspace which rows it imported and
 * their counters (the resampler may already have rewritten src_rows for the next chunk).
 * SMC at chunk boundaries: with `smc` set the forward ends with the resampler of sqair_set_smc, after the export.  Only
 * ess_frac == 1 (resample every lane at every boundary, so that the carried weights are zero and leaving them out of the
 * target is exact); the elbo_iwae of sqair_elbo summed over the chunks of a lane is then its log_evidence (a FIVO bound).
 * Refused (return -1, text in sqair_last_error, before any HIP call): a NULL carry, a B other than carry->B, state_bytes <
 * sqair_state_bytes(h, B), src_rows without state_in, a handle with sqair_set_state on, sample_from_prior, frames too large to
 * train, an smc with ess_frac != 1 (the adaptive target is not supported), a NULL SMC buffer or smc->src_rows != src_rows, an smc
 * with out->log_weights_per_timestep NULL.  Both calls are capturable (sqair_capture_begin / _end); pointers are frozen. */
typedef struct {
  const void* state_in;      /* blob to import from; NULL: every row fresh */
  void* state_out;           /* blob to export frame T' into; NULL: no export; may equal state_in */
  const int32_t* src_rows;   /* [B*K] device; NULL = identity; -1 (or out of range) = fresh */
  int64_t state_bytes;       /* >= sqair_state_bytes(h, B) */
  int32_t B;
  const SqairSmc* smc;       /* optional: resample at the end of the forward; ess_frac must be 1, smc->src_rows == src_rows */
} SqairCarry;
int sqair_forward_train_carry(SqairHandle* h, const float* flat_params, const void* packed, const float* obs, const float* noise,
                              int T, int B, const SqairCarry* carry, const SqairOutputs* out, void* train_workspace,
                              int64_t workspace_bytes, void* stream);
int sqair_backward_carry(SqairHandle* h, const float* flat_params, const void* packed, const float* obs, const float* noise,
                         const float* importance_weights, const float* vimco_signal, int T, int B, const SqairCarry* carry,
                         void* train_workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes,
                         float* flat_grad, void* stream);

/* ---- training on gappy and ragged streams: a per-frame observed mask in a carried chunk ---------------------------------------
 * A masked carried chunk is a carried chunk (SqairCarry, unchanged) plus a device mask observed[T', B] (int32, nonzero = the lane
 * has a frame), read ON THE DEVICE by both calls: one captured graph serves every mask.  A dropped frame, a lane at a lower frame
 * rate, and -- as a trailing run of zeros -- a lane whose clip ends inside the chunk (a ragged batch) are the same mechanism.
 *   Forward.  An observed (frame, lane) is untouched, bit for bit.  An unobserved one coasts exactly as sqair_set_observed defines
 *     for inference, by the same kernels: records / ids / prior state from the transition prior's draws, the temporal state held
 *     and permuted, the frame counter advanced, log_weights_per_timestep = 0, every other bound output as the inference pass writes
 *     it -- except discrete_log_prob.
 *   discrete_log_prob of a coasted (frame t, row r).  The presences of a coasted frame are DRAWN FROM p_theta, so an unbiased
 *     gradient of the chunk's bound needs their score term: the value is the sum over the N slots of
 *         pres log sigmoid(l) + (1 - pres) log sigmoid(-l),
 *     l the coasted logit (record t's presence_logit), pres the drawn presence; fp64, slots in index order.  Slots absent at t - 1
 *     of the "rnn" prior contribute 0 to rounding (l = -88).  It is written only if the lane has an observed frame LATER IN THE SAME
 *     CHUNK, else 0: a trailing run of unobserved frames influences no log weight of the chunk, its score term would be pure variance.
 *   Target.  sqair_elbo on [T', B*K] unchanged, / T' (not / the number of observed frames): VIMCO over the chunk's log weights --
 *     zero in coasted frames -- and the discrete log-probs above.
 *   Gradient.  d target / d theta with the imported state constant, as sqair_backward_carry.  A coasted frame t of row r contributes
 *     - the reparameterised draws: d what, d where of record t + 1 flow into the prior statistics of frame t (loc directly, raw scale
 *       through eps softplus'), and with prop_prior_type rw / guided into record t (the 0.1 factors of the prior's draws); d logit /
 *       d prob of the record into the logit;
 *     - the score term: g_discrete_log_prob[t, r] (presence - sigmoid(l)) into the logit of each slot;
 *     - d prior state of t + 1, through the inverse of the frame's present-first permutation, into the adjoint of the prior cell's
 *       new state; d temporal state of t + 1 through the same inverse permutation into d temporal state of t (it was held);
 *     - NOTHING from the posterior: its log-probabilities, its likelihood and its compaction are not part of a coasted frame, and
 *       the adjoints of the inference network for that (frame, row) are exactly zero.
 *   Consequences.  A chunk in which no lane is observed has target 0 and a gradient whose every entry is 0.  For one lane, a chunk
 *     of T' frames observed only in its first s frames has s / T' times the gradient of the s-frame chunk on the same frames and noise.
 *     SMC at chunk boundaries (ess_frac == 1) composes unchanged: the resampler reads zero log weights for coasted frames.
 * The frames of unobserved lanes must be FINITE (the posterior still runs on every row) and influence nothing.
 * Launches: the forward has T' + 1 kernel nodes more than sqair_forward_train_carry (k_coast_step per frame, k_coast_finish), the
 * backward T' + 1 more than sqair_backward_carry (one masking launch after the objective's adjoint, k_coast_step_bwd per frame).
 * NULL observed: the two calls ARE sqair_forward_train_carry / sqair_backward_carry, nothing more is launched.
 * The backward must be given the mask the forward ran with, unchanged in between.
 * Refused (return -1, text in sqair_last_error, before any HIP call): everything sqair_forward_train_carry / sqair_backward_carry
 * refuse (sample_from_prior among it), and a handle with a sqair_set_observed mask set.  Out of scope: a mask for the plain
 * sqair_forward_train, adaptive-ESS training, a history for training, a lane-sparse pass. */
int sqair_forward_train_carry_masked(SqairHandle* h, const float* flat_params, const void* packed, const float* obs,
                                     const float* noise, int T, int B, const SqairCarry* carry,
                                     const int32_t* observed /* device [T,B]; NULL: no mask */, const SqairOutputs* out,
                                     void* train_workspace, int64_t workspace_bytes, void* stream);
int sqair_backward_carry_masked(SqairHandle* h, const float* flat_params, const void* packed, const float* obs, const float* noise,
                                const float* importance_weights, const float* vimco_signal, int T, int B, const SqairCarry* carry,
                                const int32_t* observed /* device [T,B]; NULL: no mask */, void* train_workspace,
                                int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, float* flat_grad, void* stream);

/* ---- workspace clearing.  By default every pass starts by zero-filling the caller's workspace (60 MB for inference,
 * 308 MB for the training tape at BASELINE configs[1]: ~1-2 % of a step), so that a workspace may hold garbage and may be
 * shared between shapes.  A caller that keeps ONE workspace per (T, B, inference | training) can clear it once with
 * sqair_clear_workspace and switch the per-pass fill off with sqair_set_workspace_clearing(h, 0): every buffer is then
 * either rewritten by the pass or keeps the zeros / finite padding it never overwrites.  Re-clear after changing T or B. */
int sqair_set_workspace_clearing(SqairHandle* h, int each_pass);
int sqair_clear_workspace(SqairHandle* h, void* workspace, int64_t workspace_bytes, int T, int B, int train, void* stream);

/* Run-time options of a handle (API calls of the caller; the library reads NO environment variables):
 *   "tail_fusion" (default 1): compute the tail of slot k inside slot k + 1's VanillaRNN launch; 0 = one launch per
 *                 operation.  Results are bit-identical either way (tests/test_hip_forward.py); affects the following passes
 *                 and captures.
 *   "what_fusion" (default 1): inference passes on the launch path compute a slot's what sample (what, what_loc, what_scale:
 *                 sqair/core.py:226-229, :336-359) in the epilogue of the dense layer that produces its operands -- the glimpse
 *                 encoder's Gaussian head of a discovery slot, the temporal cell's heads of a propagation slot -- instead of in
 *                 the slot tail (csrc/sqair_glue.h: WhatArgs).  Results are bit-identical either way; re-capture graphs after
 *                 changing it.  (Training passes, the slot chain, and passes of so many particle rows -- 6000 -- that the dense
 *                 layers leave the split-K kernel always derive the sample in the tail: the option then changes nothing.)
 *   "specialised" (default 1): when the handle's dimensions are the shipped model family's (50 x 50 frames, 20 x 20 glimpses,
 *                 4 slots, n_what 50, n_hidden 256, GRU temporal and prior cells), the crops of the slot loop and the
 *                 compaction run in instantiations that have those dimensions and the launch's mode compiled in
 *                 (csrc/sqair_glue.h: sq_spec_ok).
 *                 Every other configuration runs the generic instantiations; 0 = always.  Results are bit-identical either way
 *                 (tests/test_hip_specialised.py); re-capture graphs after changing it.
 *   "specialised_mask" (default 3): which kernels "specialised" covers -- 1 crops, 2 compaction.  A measurement aid: one
 *                 kernel at a time inside one binary.
 *   "vi_target" (default 0): the learning signal sqair_elbo writes (and sqair_backward consumes) and the proxy loss in
 *                 scalars_out[2]: 0 = VIMCO, log w - control variate (sqair/targets.py:62-75: what the reference's make_target
 *                 uses); 1 = plain REINFORCE, log w (sqair/targets.py:78-89, advertised in Model.VI_TARGETS).
 *   "slot_chain" (default 0): run the strictly sequential slot launches of a frame's propagation loop, and of its discovery
 *                 loop, as ONE persistent launch each (csrc/sqair_chain.h: hand-offs through the XCD's L2, polled word by word).
 *                 Bit-identical results.  Serves the shipped cell configuration (VanillaRNN slot cell, GRU temporal cell,
 *                 n_hidden 256) up to 320 particle rows; other shapes keep one launch per op.  Set it BEFORE sizing / clearing
 *                 workspaces (the per-slot buffers are then kept apart like the training tape), and use it on a device this
 *                 process has to itself: the launch needs its 256 workgroups co-resident (another kernel occupying the CUs
 *                 makes it give up after ~20 ms with a status instead of results: sqair_chain_status).  Faster than the
 *                 launches up to ~128 particle rows (one 16-row tile per XCD), about equal at 160.
 *                 A launch reads a table of its ops that holds the operand ADDRESSES (frames, noise, parameters, workspace);
 *                 tables are cached by content in device arenas of the handle.  Passes on the same buffers reuse them; passes
 *                 on fresh buffers make new ones, and a full arena is recycled (after a stream synchronise) unless a captured
 *                 graph refers to it -- memory grows with the number of captured graphs, not with the number of passes.
 *   "slot_chain_arena_kb" (default 32768): size of one such arena; set before the first pass with the chain on.
 * Returns -2 for an unknown name. */
int sqair_set_option(SqairHandle* h, const char* name, int value);
/* Status of the slot chain's launches of the last pass on `workspace` (synchronises `stream`): 0 = all completed (or the chain is
 * off for this shape), else the first non-zero status (1 = an operand never arrived, 3 = the workgroups were not co-resident,
 * 6 = an earlier launch of the pass had failed); the text is in sqair_last_error. */
int sqair_chain_status(SqairHandle* h, void* workspace, int T, int B, int train, void* stream);
/* Debug mode of the reference (`debug=True` -> validate_args / allow_nan_stats=False on its distributions,
 * sqair/core.py:226, :261, sqair/modules.py:318-320; a TF runtime error inside sess.run): checks x[0:n] for NaN / Inf on
 * `stream`, SYNCHRONISES it, and returns -5 with "non-finite values in <what>: count, first index" in sqair_last_error.
 * flag_dev: caller-owned device int32[2] scratch. */
int sqair_check_finite(SqairHandle* h, const float* x, int64_t n, const char* what, int32_t* flag_dev, void* stream);
/* The same mode's argument validation of the Normal distributions: the posterior scales of `what` and `where` of EVERY propagation
 * and discovery slot of the last pass on `workspace` must be positive and finite -- also of slots the presence mask later removes
 * from the log-weights (which sqair_check_finite on the log-weights cannot see).  Synchronises; -5 + text on failure. */
int sqair_check_scales(SqairHandle* h, void* workspace, int T, int B, int train, int32_t* flag_dev, void* stream);

/* ---- per-dispatch timeline (measurement; bench.py's roofline, tools/timeline.py) -----------------------------------------
 * libsqair_hip_timeline.so is THIS library compiled with -DSQAIR_TIMELINE: every kernel takes one more argument and every
 * wave stores {start, end} of its life on the 100 MHz device wall clock (s_memrealtime) into its own 16-byte slot of `buf`.
 * Between _begin and _end every launch issued through the library (eagerly or into a capture) is assigned the next slot
 * range (an eager launch a fresh one every time); replaying a graph captured in between re-stamps the same slots.  _count /
 * _end return the number of records; _record(i)
 * gives kernel name, offset of the range in 8-byte words, waves (= pairs) and workgroups.  Reduce min(start) / max(end) over
 * the pairs of a record for first-wave-start / last-wave-end of that dispatch (zero pairs = padding).  A stamped step runs
 * ~3 % slower than the product library's (measured).  The production library returns -3 from
 * _begin (sqair_timeline_available() == 0) and carries none of this in its kernels. */
int sqair_timeline_available(void);
int sqair_timeline_begin(SqairHandle* h, void* buf, int64_t bytes);
int sqair_timeline_count(const SqairHandle* h);  /* records so far (recording continues); -4 once the stamp buffer has overflowed */
int sqair_timeline_end(SqairHandle* h);
int sqair_timeline_record(const SqairHandle* h, int i, const char** kernel, int64_t* offset_u64, int* waves, int* workgroups);

/* Generation modes (sqair/sqair_modules.py:157-170, :294-302, sqair/seq.py:198-200).  With
 * cfg.sample_from_prior the propagation posterior log-probabilities are evaluated at samples of the propagation PRIOR, and
 * in frames t > cfg.generate_after those samples replace what / where / presence of the propagated objects, discovery's
 * what ~ N(0, I), where ~ its (recurrent) prior and presence = 0.  The extra draws come from `gen_noise`, same layout
 * and meaning as `noise` ([T, B*K, 2, N, 4 + n_what + 1]); the pointer is remembered by the handle and used by the
 * following forward calls.  Forward / inference only. */
int sqair_set_generation_noise(SqairHandle* h, const float* gen_noise);
/* Device-side noise for one pass: fills noise[T, B*K, 2, N, 4 + n_what + 1] with eps ~ N(0,1) / u ~ U[0,1) (last entry
 * of every slot) from Philox4x32-10 keyed by (seed, step, position in the GLOBAL batch): a rank that owns sequences
 * [b0, b0 + B) of a global batch of global_B draws exactly the rows one GPU would have drawn for them.  Replaces the
 * tfd `.sample()` calls the reference makes inside its graph (sqair/core.py:226, sqair/modules.py:60, :485). */
int sqair_fill_noise(SqairHandle* h, float* noise, int T, int B, int global_B, int b0, uint64_t seed, uint64_t step,
                     void* stream);
/* Graph capture of any sequence of the calls above on one stream (the training step up to the gradient all-reduce
 * is ~3000 short dependent launches): _begin, issue the calls, _end(slot 0..3) -> node count (>= 0) or error (< 0);
 * _launch replays the slot.  Captured calls keep the pointers they were given. */
int sqair_capture_begin(SqairHandle* h, void* stream);
int sqair_capture_end(SqairHandle* h, void* stream, int slot);
int sqair_capture_launch(SqairHandle* h, int slot, void* stream);
/* flat_grad += l2 * flat_params: the l2_reg term of Model.make_target (sqair/targets.py:31-35, sqair/model.py:160). */
int sqair_add_l2_grad(SqairHandle* h, const float* flat_params, float* flat_grad, int64_t n, float l2, void* stream);
/* Fused optimiser step on the flat buffers: tf.train.RMSPropOptimizer(lr, momentum=0.9) as used by the
 * reference driver (sqair/scripts/experiment.py:140; TF defaults decay 0.9, epsilon 1e-10, ms initialised to 1):
 * ms <- decay ms + (1-decay) g^2; mom <- momentum mom + lr g / sqrt(ms + eps); theta <- theta - mom, with
 * g = grad_scale * flat_grad (grad_scale = 1/world after the data-parallel all-reduce(sum)). */
int sqair_rmsprop_step(SqairHandle* h, float* flat_params, const float* flat_grad, float* ms, float* mom, int64_t n,
                       float lr, float decay, float momentum, float epsilon, float grad_scale, void* stream);
/* Dense layer backward on the kernels of the training step (test helper): y = act(x W + b) forward; given dy returns
 * dx [M,K], dw [K,N] (reference [in,out] layout) and db [N].  dw / db take the route sqair_backward gives a block: the
 * grouped weight-gradient kernel, or a launch of their own when x's rows are not 16-byte aligned (Kdim % 4 != 0). */
int sqair_linear_bwd_test(SqairHandle* h, const float* x, const float* w, const float* y, const float* dy, float* dx,
                          float* dw, float* db, int M, int Kdim, int Ndim, int act, void* scratch,
                          int64_t scratch_bytes, void* stream);

/* ---- the dense family's operand contract and the routed dX launcher, one launch each (test helpers) ------------------------
 * Both entries hand the caller's operand pointers, pitches and divisors to the launcher UNCHANGED (no staging copy): the caller
 * owns alignment (segment / dpre base on 16 bytes, pitch a multiple of 4 floats -- otherwise the launcher refuses, -5, and
 * nothing is launched), the readable and finite round_up(width, 4) floats of every operand row, and ceil(M / rdiv) rows behind a
 * row divisor.  Only the weights are packed into `scratch`.  Errors carry the entry's name (sqair_last_error). */
typedef struct SqairDenseSeg {
  const float* p;          /* row r of the layer reads p + (r / rdiv) * ld */
  int32_t ld;              /* 0 = one broadcast row */
  int32_t width;           /* inputs taken from this segment */
  int32_t rdiv;            /* >= 1 */
} SqairDenseSeg;
/* out[m, n] = act(sum_i x_i[m / rdiv_i] W_i + b + (n < add_n ? add[m / add_rdiv, n] : 0))[n] * scale * *scale_ptr, n < N; act = act_a
 * for n < act_split, act_b otherwise (codes of sqair_linear_test).  w: dense row-major [sum(width), N], segment after segment;
 * b [N] or NULL; add / scale_ptr NULL = none; out_ld >= N.  scratch >= 4 * (2 * nt * kc * 256 + 32 * nt + 256) bytes with
 * kc = sum_i ceil(width_i / 16), nt = ceil(N / 16). */
typedef struct SqairDenseContract {
  int32_t nseg;            /* 1..4 */
  SqairDenseSeg seg[4];
  const float* w;
  const float* b;
  const float* add;
  int32_t add_ld, add_n, add_rdiv;
  int32_t act_a, act_b, act_split;
  float scale;
  const float* scale_ptr;
  float* out;
  int32_t out_ld, M, N;
  void* scratch;
  int64_t scratch_bytes;
} SqairDenseContract;
int sqair_linear_contract_test(SqairHandle* h, const SqairDenseContract* c, void* stream);

/* The routed dX GEMM of the training step: v = dpre [M, width] (pitch ld) W^T * *scale_ptr for the forward matrix w [Kdim, width];
 * columns [n0, n1) of v (n0 a multiple of 16) go to range i: dst[m, n - n0] = dact(v + add[m, n - n0], saved[m, n - n0]) and the same
 * to dst2; add may be dst (accumulate); saved = the producing layer's saved OUTPUT, its activation act_a for n - n0 < act_split,
 * act_b otherwise; every pointer but dst optional.  gru.mode 1 / 2: the GRU gate adjoints in the epilogue instead (one range
 * [0, nh) without saved): mode 1, g = v: dpre1[:, 0:nh] = g (hc - h) z (1 - z), dpre1[:, 2nh:3nh] = g z (1 - hc^2), d_h (+)= g (1 - z)
 * with z = g0, hc = g1, h = hprev; dup[:, 0:nh] and dup[:, dup_h_off:] (dup_h_off >= 0) receive second copies of the two; mode 2,
 * g = v: dpre1[:, nh:2nh] = dup = g h r (1 - r), d_h += g r with r = g0.  Returns the launcher's code: -5 (alignment, pitch, a range
 * start off 16 columns, nranges outside 1..3), -6 (a GRU block with a saved pointer, with more than the one range [0, nh), or
 * deeper than the build's instantiations: width > 256 on the product library).
 * scratch >= 4 * (2 * nt * kc * 256 + 256) bytes with kc = ceil(width / 16), nt = ceil(Kdim / 16). */
typedef struct SqairDxRange {
  int32_t n0, n1;
  float* dst; int32_t dst_ld;
  float* dst2; int32_t dst2_ld;
  const float* add; int32_t add_ld;
  const float* saved; int32_t saved_ld;
  int32_t act_a, act_b, act_split;
} SqairDxRange;
typedef struct SqairDxGru {
  int32_t mode;
  const float* g0; int32_t g0_ld;
  const float* g1; int32_t g1_ld;
  const float* hprev; int32_t h_ld;
  float* dpre1; int32_t dp_ld;
  float* d_h; int32_t dh_ld, acc_dh;
  float* dup; int32_t dup_ld, dup_h_off;
  int32_t nh;
} SqairDxGru;
typedef struct SqairDxTest {
  const float* dpre; int32_t ld, width, M;
  const float* w; int32_t Kdim;
  const float* scale_ptr;
  int32_t nranges;
  SqairDxRange r[3];
  SqairDxGru gru;
  void* scratch;
  int64_t scratch_bytes;
} SqairDxTest;
int sqair_linear_dx_test(SqairHandle* h, const SqairDxTest* t, void* stream);

/* ---- the element-wise adjoints of the slot loop, one launch each (test helpers) -----------------------------------------------
 * The kernels that sit between the dX GEMMs in the reverse sweep of sqair_backward, on caller-owned device buffers that reach the
 * pass's own launchers UNCHANGED.  The dimensions (R = B * k_particles rows, N slots, n_what, n_hidden, the frame, the glimpse), the
 * record layout and every parameter offset (steps predictors, scale offsets, Cholesky factor) are the handle's, derived by the
 * expressions the pass uses; the caller chooses mode, slot, B, the pitches and which optional outputs exist.  `flat` / `flat_grad`
 * are parameter buffers in the kernels' own layout (sqair_debug_padded_count floats: the caller's layout unless n_hidden is
 * padded); records are [R][N][W] with the columns sqair_compact_test_layout reports; noise is one frame's [R][2][N][4 + n_what + 1]
 * (phase 0 propagation, 1 discovery).  A refusal (-1: a NULL required pointer, a slot outside [0, N), a pitch below the width, a
 * frame that cannot be trained) carries the entry's name in sqair_last_error and launches nothing; otherwise the launcher's code,
 * after a stream synchronise.
 *
 * sqair_slot_tail_bwd_test (k_slot_tail_bwd): presence logit -> steps predictor -> `what` sample; reads d_rec_new[LOGIT, WHAT,
 *   WHAT_LOC, WHAT_SCALE] of the slot, the previous presence (discovery: the record of slot - 1, 1 for slot 0; propagation:
 *   rec_prev), s1h [R][n_hidden / 2] the saved hidden activations, enc [R][2 n_what] = (loc, scale) of the glimpse encoder, and in
 *   propagation hraw [R][5 n_what] (what-head loc, raw scale, three raw gates) and rec_prev[WHAT].  Writes d_s1pre (and the copy
 *   d_s1pre2, optional), d_raw_out [R][dr_ld] (one float per row), d_rec_new[WHAT] (the sample's total gradient), d_enc [R][2 n_what]
 *   (enc_pre 1, discovery: the scale half as the gradient of the head's pre-activation), and in propagation d_hraw [R][5 n_what] and
 *   d_rec_prev[WHAT] += .  rec_prev, d_rec_prev, hraw and d_hraw are required in propagation only. */
typedef struct SqairSlotTailBwdTest {
  int32_t is_disc, slot, B, enc_pre;
  const float* rec_prev; const float* rec_new;
  float* d_rec_new; float* d_rec_prev;
  const float* s1h; int32_t s1h_ld;
  const float* hraw; int32_t h_ld;
  const float* enc; int32_t enc_ld;
  const float* noise;
  const float* flat;
  float* d_s1pre; int32_t ds_ld;
  float* d_s1pre2; int32_t ds2_ld;
  float* d_raw_out; int32_t dr_ld;
  float* d_enc; int32_t de_ld;
  float* d_hraw; int32_t dh_ld;
} SqairSlotTailBwdTest;
int sqair_slot_tail_bwd_test(SqairHandle* h, const SqairSlotTailBwdTest* t, void* stream);

/* sqair_crop_chain_bwd_test (k_crop_chain_bwd): d glimpse -> d where -> the where sample's adjoint.  mode 1 (crop #1 of
 *   propagation): ALL N slots in one launch (`slot` ignored), where logits = rec_prev[WHERE] + 0.1 wb; row r, slot k reads g_out row
 *   r * g_row_mul + g_row_add + k and mask row r * mask_row_mul + mask_row_add + k (both multipliers >= N); writes d_wb
 *   [R * N][wb_ld] and d_rec_prev[WHERE] += .  mode 2 / 3 (crop #2 of propagation / discovery): one slot, where = rec_new[WHERE];
 *   reads d_rec_new[WHERE, WHERE_LOC, WHERE_SCALE], tp [R][8] the saved transform output, the phase's noise; writes d_tp [R][8],
 *   d_rec_new[WHERE] (the sample's total gradient) and, mode 2, d_rec_prev[WHERE] += .  mask (optional, [rows][G * G]) multiplies the
 *   glimpse; then d_mask += , and with mask_dact 1 the sum is written times mask (1 - mask).  d_t2 (optional, modes 2 / 3): the
 *   adjoint of the transform's output layer in the same launch, d_t2[r][j] = (sum_o d_tp[r][o] w3[j][o]) elu'(t2[r][j]) with w3
 *   [n_hidden][8] and t2 the saved hidden activations.  img: [B] frames, each padded with zeros to a multiple of 4 floats. */
typedef struct SqairCropChainBwdTest {
  int32_t mode, slot, B, mask_dact;
  const float* img;
  const float* rec_prev; const float* rec_new;
  float* d_rec_prev; float* d_rec_new;
  const float* wb; int32_t wb_ld;
  float* d_wb;
  const float* mask; int32_t mask_row_mul, mask_row_add;
  float* d_mask;
  const float* g_out; int32_t g_row_mul, g_row_add;
  const float* tp; int32_t tp_ld;
  float* d_tp; int32_t dtp_ld;
  const float* noise;
  const float* flat;
  const float* w3;
  const float* t2; int32_t t2_ld;
  float* d_t2; int32_t dt2_ld;
} SqairCropChainBwdTest;
int sqair_crop_chain_bwd_test(SqairHandle* h, const SqairCropChainBwdTest* t, void* stream);

/* sqair_where_param_grads_test (k_where_param_grads): the batched reduction over all T * R * N (frame, row, slot) uses into the ten
 *   entries of prop.cholesky_scale and the two transform.scale_offset scalars, ADDED onto flat_grad.  d_tp [2 phases][T * R * N][tp_ld]
 *   (columns 4:8 are summed); d_rec_p / rec_p [T][R][N][W] (d where total, where_scale); noise [T][R][2][N][4 + n_what + 1]. */
typedef struct SqairWhereParamGradsTest {
  int32_t T, B;
  const float* d_tp; int32_t tp_ld;
  const float* d_rec_p; const float* rec_p;
  const float* noise;
  float* flat_grad;
} SqairWhereParamGradsTest;
int sqair_where_param_grads_test(SqairHandle* h, const SqairWhereParamGradsTest* t, void* stream);

/* sqair_gru_gates_bwd_test (k_gru_bwd_a, then k_gru_bwd_b): the gate adjoints of the slot RNN's GRU over `rows` rows of n_hidden
 *   units.  Stage A from d_hn = d h': dpre1[:, 0:nh] = d(z pre-activation), dpre1[:, 2nh:3nh] = d(candidate pre-activation), d_h (+)=
 *   the direct part (accumulate_dh 1 adds); dup_z (optional) receives the first at column 0 and the second at dup_h_off (>= 0).
 *   Stage B from d_rh = d(r h): dpre1[:, nh:2nh] = d(r pre-activation) (copy: dup_r, optional), d_h += d_rh r.  z, r, hc: the saved
 *   gate OUTPUTS; hprev with h_ld 0 is one broadcast row. */
typedef struct SqairGruGatesBwdTest {
  int32_t rows, accumulate_dh;
  const float* d_hn; int32_t dhn_ld;
  const float* z; int32_t z_ld;
  const float* r; int32_t r_ld;
  const float* hc; int32_t hc_ld;
  const float* hprev; int32_t h_ld;
  const float* d_rh; int32_t drh_ld;
  float* dpre1; int32_t dp_ld;
  float* d_h; int32_t dh_ld;
  float* dup_z; int32_t dupz_ld, dup_h_off;
  float* dup_r; int32_t dupr_ld;
} SqairGruGatesBwdTest;
int sqair_gru_gates_bwd_test(SqairHandle* h, const SqairGruGatesBwdTest* t, void* stream);

/* ---- the forward kernels of the slot loop, one launch each (test helpers) ----------------------------------------------------------
 * k_crop_row, k_slot_tail, k_rnn_tail and k_linear_what under the rules of the adjoint entries above: caller-owned device buffers reach the
 * pass's own launchers UNCHANGED, through the argument builder and launch helpers the pass calls; dimensions, record layout and
 * parameter offsets are the handle's; a refusal is -1, names the entry in sqair_last_error and launches nothing; otherwise the
 * launcher's code, after a stream synchronise.  `flat` as above; `packed` is sqair_pack_params' output for these parameters.
 * Records [R][N][W], noise one frame's [R][2][N][4 + n_what + 1] (phase 0 propagation, 1 discovery), R = B * k_particles.
 *
 * sqair_slot_crop_test (k_crop_row; mode 1 = crop #1 of propagation, ALL N slots of a row in one launch, `slot` ignored; mode 2 / 3 =
 *   crop #2 of a propagation / discovery slot).  One workgroup per (row, slot); with B a multiple of 8 workgroup i serves row
 *   ((i / 8 / K) * 8 + i % 8) * K + (i / 8) % K, else row i.  specialised 0: the generic instantiation; 1: the instantiation with the
 *   shipped family's dimensions compiled in, where the handle has them, the frame is staged, modes 1 / 2 have a mask, mode 3 none,
 *   and modes 2 / 3 come with t2 -- otherwise the generic one all the same.  Frames up to 4096 pixels are staged in LDS.
 *   READS  img [B] frames at a pitch of H * W rounded up to 4 floats: the H * W pixels of frame r / K, not the padding; mask
 *          (optional) row r * mask_row_mul + mask_row_add (+ slot in mode 1), G * G floats.
 *          mode 1: rec_prev(r, slot)[WHERE], wb [(r * N + slot)][4]; where logits = rec_prev[WHERE] + 0.1 wb.
 *          modes 2 / 3: noise[r][phase][slot][0 : 4] (phase 0 / 1); tp [R][loc 4 | raw scale 4], or with t2 [R][n_hidden] (16-byte
 *          aligned rows) the transform's output layer w3 = {w [n_hidden][8], b [8]} (16-byte aligned) evaluated in the launch;
 *          of flat disc.transform.scale_offset (mode 3) / prop.transform.scale_offset and the ten prop.cholesky_scale (mode 2);
 *          mode 2 also rec_prev(r, slot)[WHERE].  mode 3: loc = tp[0:4], scale = softplus(raw + offset) + 1e-2, where = loc +
 *          scale eps.  mode 2: loc = rec_prev[WHERE] + tp[0:4], scale = softplus(raw + offset - 1) + 1e-2, where = loc + L eps with
 *          L = fill_triangular(cholesky) * scale[:, None] + diag(scale).
 *   WRITES out row r * out_row_mul + out_row_add (+ slot in mode 1): the G x G glimpse (times the mask); modes 2 / 3:
 *          rec_new(r, slot)[WHERE, WHERE_LOC, WHERE_SCALE]; with t2 and tp_out: tp_out [R][8] = the output layer's result.  Nothing
 *          else: no other column or slot of a record, no other row of out / tp_out.  rec_prev is never written. */
typedef struct SqairSlotCropTest {
  int32_t mode, slot, B, specialised;
  const float* img;
  const float* rec_prev; float* rec_new;
  const float* wb; int32_t wb_ld;
  const float* tp; int32_t tp_ld;
  const float* t2; int32_t t2_ld;
  const float* w3;
  const float* noise;
  const float* flat;
  const float* mask; int32_t mask_row_mul, mask_row_add;
  float* out; int32_t out_row_mul, out_row_add;
  float* tp_out; int32_t tp_out_ld;
} SqairSlotCropTest;
int sqair_slot_crop_test(SqairHandle* h, const SqairSlotCropTest* t, void* stream);

/* sqair_slot_tail_test.  Without the RNN block (out NULL): k_slot_tail<what_done>, one workgroup per 16 rows.  Per row r (a ragged
 *   last tile re-reads row R - 1 and stores nothing for it):
 *   READS  noise[r][phase][slot][4 + n_what] (the uniform u); the previous presence -- propagation: rec_prev(r, slot)[PRES];
 *          discovery: rec_new(r, slot - 1)[PRES], slot 0: none, it is 1 -- ; s1p [R][n_hidden / 2]; of `packed` the phase's *_S1 pack
 *          (the `what` rows of steps.l0.w); of `flat` steps.l1.w [n_hidden / 2] and steps.l1.b.
 *          what_done 0: enc [R][loc n_what | scale n_what], noise[..][4 : 4 + n_what]; propagation also hraw [R][5 n_what] (what-head
 *          loc, raw scale, raw forget / input / temporal gate) and rec_prev(r, slot)[WHAT].
 *          what_done 1 (product library only): rec_new(r, slot)[WHAT] instead; enc, hraw, the `what` noise and rec_prev[WHAT] are
 *          NOT read (they may be NULL or hold NaN).
 *   WRITES rec_new(r, slot)[PRES, LOGIT, PROB]; what_done 0: also [WHAT, WHAT_LOC, WHAT_SCALE][0 : n_what]; s1h_out [R][n_hidden / 2]
 *          (optional) = elu(s1p + what W).  No other column of the record, no other slot, no row beyond R.
 *   A row whose previous presence is 0 gets logit = 0 * raw - 88 = -88 exactly (raw must be finite), presence 0, prob = sigmoid(-88);
 *   its sample and s1h_out are written like any other row's.  presence = (u < prob) * previous presence.
 * With the RNN block (out set; product library, VanillaRNN slot cell, n_hidden 128 / 256, option tail_fusion on, slot + 1 < N):
 *   k_rnn_tail = the same tail inside the NEXT slot's layer, out [R][n_hidden] = tanh([z | hid] W + b + add) on the phase's
 *   L_PROP_RNN / L_DISC_RNN pack, z = rec_new(r, slot)[WHERE .. LOGIT] with the fresh tail results.  Every workgroup (16 rows x 16
 *   or 32 columns) re-derives the tail of its rows and additionally READS rec_new(r, slot)[WHERE] (written by the slot's crop; must
 *   be finite), hid [R][n_hidden] (16-byte aligned rows), add [R][n_hidden], the pack and its bias.  Only the column-tile-0
 *   workgroups WRITE the record and s1h_out (exactly what k_slot_tail writes); all write their tile of `out`. */
typedef struct SqairSlotTailTest {
  int32_t is_disc, slot, B, what_done;
  const float* hraw; int32_t h_ld;
  const float* enc; int32_t enc_ld;
  const float* rec_prev; float* rec_new;
  const float* noise;
  const float* s1p; int32_t s1p_ld;
  float* s1h_out; int32_t s1h_ld;
  const float* flat; const float* packed;
  const float* hid; int32_t hid_ld;      /* the optional RNN block */
  const float* add; int32_t add_ld;
  float* out; int32_t out_ld;
} SqairSlotTailTest;
int sqair_slot_tail_test(SqairHandle* h, const SqairSlotTailTest* t, void* stream);

/* sqair_linear_what_test (k_linear_what<n_hidden / 64, mode> on the L_WHAT_HEAD_I / L_PROP_HEADS_I pack; M = B * k_particles rows;
 *   refused on the wide library and where n_hidden is neither 128 nor 256).  One workgroup per 16 rows x 16 interleaved columns.
 *   READS  x [M][n_hidden] (16-byte aligned rows, x_ld a multiple of 4), the pack and its bias, noise[r][phase][slot][4 : 4 + n_what]
 *          (phase 1 for mode 0, 0 for mode 1); mode 1 also enc [M][loc n_what | scale n_what] and rec_prev(r, slot)[WHAT].
 *   WRITES rec_new(r, slot)[WHAT, WHAT_LOC, WHAT_SCALE][0 : n_what] and nothing else: mode 0 (discovery) loc = x W_loc + b,
 *          scale = softplus(x W_scale + b) + 1e-2; mode 1 (propagation) the gated mixture of the tail; what = loc + scale eps.
 *   The result has the bits of the plain head layer (L_WHAT_HEAD / L_PROP_HEADS) on the split-K kernel followed by the tail. */
typedef struct SqairLinearWhatTest {
  int32_t mode, slot, B;
  const float* x; int32_t x_ld;
  const float* noise;
  const float* enc; int32_t enc_ld;
  const float* rec_prev; float* rec_new;
  const float* packed;
} SqairLinearWhatTest;
int sqair_linear_what_test(SqairHandle* h, const SqairLinearWhatTest* t, void* stream);

/* ---- the log-probability kernels, one launch each (test helpers) -----------------------------------------------------------------
 * k_logprob (section H of the forward pass) and its adjoint k_logprob_bwd (H^T, the head of sqair_backward's reverse sweep), under
 * the rules of the slot-loop entries above: caller-owned device buffers reach the two launchers UNCHANGED; dimensions, SqairConfig,
 * record layout and every parameter offset are the handle's; the caller chooses B, T, the pstats pitch, the time source (t_row [R]
 * per-row frame counters, or NULL: t_global / t_global0; frame f of row r has time t_row[r] + f) and which optional outputs exist.
 * A refusal (-1: a NULL required pointer, B < 1, T < 1, ps_ld < 9 + 2 n_what or so large that the row no longer fits 150 KB of LDS,
 * for the adjoint a frame that cannot be trained) carries the entry's name in sqair_last_error and launches nothing; otherwise the
 * launcher's code, after a stream synchronise.  R = B * k_particles, M = R * N; records [frames][R][N][W] (columns:
 * sqair_compact_test_layout); pstats [T][M][ps_ld] = the prior's raw statistics [logit | where_loc 4 | what_loc n_what |
 * where_scale 4 | what_scale n_what]; spre [T][R][128] the where prior's conditioning pre-activation without the expected-steps
 * row (required with rec_where_prior only); flat / flat_grad in the kernels' own layout (sqair_debug_padded_count floats).
 *
 * sqair_logprob_test (k_logprob, gen = NULL: the generation modes stay with sqair_forward).  READS, per (frame, row): of rec_p
 *   WHERE, WHAT[0:n_what], PRES, LOGIT, WHERE_LOC, WHERE_SCALE, WHAT_LOC, WHAT_SCALE; of rec_d the same without LOGIT, plus PROB; of
 *   rec_prev [T][R][N][W] (frame f: the merged records of f - 1) PRES, and under rw / guided only WHERE, WHAT, LOGIT;
 *   pstats columns [0, 9 + 2 n_what) (the loc columns 1 .. 4 + n_what not under rw); spre and the where-prior parameters
 *   (disc.rn.i2h, .h2h, .readout, .init_sample, row 4 + n_hidden of disc.rn.cond.w) with rec_where_prior; disc.steps_prior.*,
 *   disc.step_prior_bias and (where the time is > 0) disc.step_prior_timestep_bias with the categorical step prior;
 *   prop.cholesky_scale.  The row's records and statistics are staged whole, so every other word of them may hold anything, NaN
 *   included; the fields of an ABSENT slot are read and multiplied by the zero mask: they must be finite.  WRITES qz, pz, disc_lp
 *   [T][R] at frame f, and of `out` (optional, as every pointer in it) at frame t + f: the eight per-slot log-probs, prop_prob,
 *   prop_pres, disc_pres [..][N], disc_prob [..][N + 1], prop / disc (prior) log-probs, step_log_prob, discrete_log_prob and the
 *   two step counts; nothing else of `out` is touched. */
typedef struct SqairLogprobTest {
  int32_t B, T, t, t_global;
  const int32_t* t_row;
  const float* rec_p; const float* rec_d; const float* rec_prev;
  const float* pstats; int32_t ps_ld;
  const float* spre;
  const float* flat;
  float* qz; float* pz; float* disc_lp;
  const SqairOutputs* out;
} SqairLogprobTest;
int sqair_logprob_test(SqairHandle* h, const SqairLogprobTest* t, void* stream);

/* sqair_logprob_bwd_test (k_logprob_bwd): the adjoint of sum over (frame, row) of g_lw (pz - qz) + g_dl disc_lp.  READS what
 *   k_logprob reads, with two differences: rec_m is [T + 1][R][N][W] (frame f reads rec_m[f]; only its z segment WHERE .. LOGIT is
 *   staged, frame T not at all), and all fifteen small-parameter segments are staged whatever the flags (an unused one may hold NaN).
 *   g_lw, g_dl [T][R].  ACCUMULATES (+=, float atomics, exact zeros skipped): d_rec_p in WHERE, WHAT[0:n_what], LOGIT, WHERE_LOC,
 *   WHERE_SCALE, WHAT_LOC, WHAT_SCALE; d_rec_d in the same columns (its LOGIT holds the gradient of logit(PROB) through the
 *   number-of-steps posterior); d_rec_m[f] in LOGIT (rw / guided: also of slots absent at f - 1, through the expected number of
 *   steps) and WHERE / WHAT[0:n_what] (rw / guided), frame T untouched; flat_grad inside the fifteen segments prop.cholesky_scale,
 *   disc.rn.{readout, i2h, h2h}.{w, b}, row 4 + n_hidden of disc.rn.cond.w, disc.rn.init_sample, disc.steps_prior.{l0, l1}.{w, b},
 *   disc.step_prior_bias, disc.step_prior_timestep_bias and nowhere else.  WRITES (=): d_pstats [T][M][ps_ld] over the full pitch,
 *   zeros outside the used columns (rw: the loc columns are zeros too); d_spre [T][R][128], zeros without rec_where_prior.  Masks
 *   multiply, they do not select: an absent slot's fields must be finite. */
typedef struct SqairLogprobBwdTest {
  int32_t B, T, t_global0, ps_ld;
  const int32_t* t_row;
  const float* rec_p; const float* rec_d; const float* rec_m;
  const float* pstats; const float* spre;
  const float* g_lw; const float* g_dl;
  float* d_rec_p; float* d_rec_d; float* d_rec_m;
  float* d_pstats; float* d_spre;
  const float* flat; float* flat_grad;
} SqairLogprobBwdTest;
int sqair_logprob_bwd_test(SqairHandle* h, const SqairLogprobBwdTest* t, void* stream);

/* Which kernel family the two dense launchers chose, counted on the host per process (launches issued or captured so far), at the
 * point of the choice: out[0:n] receives the first n of the SQAIR_DENSE_ROUTES counts below, the return value is their number.
 *   forward (sq_launch_linear):  0 split-K (k_linear) | 1 32 x 32 tiles (k_linear_t2) | 2 k_linear_rows | 3 k_linear_mt |
 *                                4 k_linear_lds | k_linear_big with wave tile 5 2 x 2 | 6 3 x 2 | 7 3 x 3 | 8 4 x 2
 *   dX (sq_launch_linear_dx):    k_linear_dx<NCH> with NCH = 9 1 | 10 2 | 11 3 | 12 4 | 13 5 | 14 6 | 15 7 | 16 8 | 17 9 | 18 12 |
 *                                19 18 | 20 32 x 32 tiles (k_linear_dx_t2) | 21 GRU mode 1 | 22 GRU mode 2
 *   forward, added later:        23 one-round strip (k_linear_strip; the split-K kernel's bits)
 * A refused launch (-5, -6) and an empty one count nothing. */
#define SQAIR_DENSE_ROUTES 24
int sqair_debug_dense_routes(int64_t* out, int n);

#ifdef __cplusplus
}
#endif
#endif /* SQAIR_HIP_H */
