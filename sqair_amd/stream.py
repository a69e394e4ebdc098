"""Stateful streaming inference: a video fed as its frames arrive, object identities and latent states carried from call to call.

``SqairStream(core, B)`` owns a state blob on the device (include/sqair_hip.h: sqair_state_bytes / sqair_set_state) and runs the
T'-frame inference pass of ``core`` (frames_per_step = T') once per ``step()``: each particle row starts from the state the
previous step left and the pass writes its new state back into the same blob.  With ``use_graph`` ONE HIP graph of that pass is
captured on the first step and replayed on every later one -- the rows' frame counters live on the device, so the same graph
serves frame 0, frame 1000 and a batch in which some lanes were just reset.

Stepping a sequence in chunks gives the results of one pass over the whole sequence, bit for bit, when the chunks see the same
noise (tests/test_stream_state.py).  Without explicit ``noise`` a step draws its own from the library's Philox generator keyed by
(seed, frame index of the step's first frame, row): NOT the draws a whole-sequence pass with the same seed makes (that one keys
every frame of the pass by one step index), so results agree with such a pass only in distribution.

With ``resample="systematic"`` the stream is an adaptive particle filter run inside the pass (include/sqair_hip.h:
sqair_set_smc): the per-frame log weights are the incremental importance weights of a filter whose proposal is the inference
network, and a kernel at the end of every pass computes each lane's ESS and log evidence and, when ESS < ess_frac * K (always for
ess_frac = 1, never for 0), resamples the lane's particles systematically by writing the source map of the next step -- no host
decision, so the one captured graph still serves every frame.  Resampling happens at step boundaries: frames_per_step = 1 gives
per-frame SMC.  The uniform of a lane is the step's ``uniforms[b]`` when given, else Philox keyed by (``seed``, lane, frame
counter).  ``log_weight_sum`` is then the device accumulator of each row's log weight SINCE ITS LANE'S LAST RESAMPLING (zeroed
there; the evidence banked at resamplings is ``log_z``), and ``step()`` adds ``ess``, ``resampled``, ``log_evidence`` (the SMC
estimate of log p(x_1..t) per lane) and ``ancestors`` (the source map of the next step) to its outputs.

``forecast(F)`` answers the tracker's next question -- where will the objects be, what will the next frames look like: it rolls the
generative prior F frames forward from the rows the next ``step()`` would start from (include/sqair_hip.h: sqair_forecast), with
discovery empty, and renders every frame.  Per particle it returns the sampled objects and the decoder's canvas; per lane the
predictive mean canvas and expected object count under the particles' weights.  It writes nothing the steps read: forecasting
between steps leaves every step's results unchanged.

With ``history=L`` the last L steps are kept in a ring on the device, written by one more kernel of the pass (include/sqair_hip.h:
sqair_set_history), and ``tracks(lag)`` traces them on the device into trajectories (sqair_history_trace): as soon as a lane
resamples, row r of this step no longer continues row r of the last one, so the track of an object is the path through the source
maps -- the surviving particles' trajectories, the fixed-lag smoothing distribution of the filter -- and, because compaction moves
objects between slots, a table keyed by object id.  No per-step copy to the host, no host-side genealogy.

With ``missing=True`` a step takes ``observed`` [T', B]: lanes without a frame -- a dropped frame, a slower camera, a known occluder --
coast on the prior inside the pass (include/sqair_hip.h: sqair_set_observed).  Their particles are proposed from the transition
prior, as ``forecast`` would, their temporal states held, their weights left alone, and time advances; the mask lives on the device,
so the one captured graph serves every pattern of present and missing lanes.  Feeding a blank frame instead would let the inference
network "see" an empty scene and kill the objects.

With ``estimate=True`` a step also returns ``out["lane"]``: one answer per lane and frame from the K particles, and its followers
say more about it, each one more kernel of the pass -- ``estimate_layers`` which pixels each object occupies, ``identity`` a track id
that stays on an object (``motion``: with a velocity filter per track inside the same kernel, sqair_set_motion; ``tracklog``: the
last frames of every lane by lane_id in a ring on the device, ``track_log()`` their smoothed trajectories, sqair_set_tracklog; ``tracklog_truth``: the steps' truth kept beside it, ``track_log(score=True)`` the trajectories scored against it, sqair_lane_tracklog_score), ``score`` the CLEAR-MOT events against a step's ``truth`` (``score()``, ``identities()``; ``score_match`` / ``identity_match`` =
"optimal": their per-frame matching as keep + optimal, sqair_set_lane_match), ``score_idf`` the identity overlap table
IDF1 is solved from (``idf_score()``), ``score_hota`` the clip log HOTA is solved from (``hota_score()``); ``forecast`` and
``tracks`` with ``lane=True, truth=...`` score the lane forecast and the lane tracks (``trajectory_score(kind)``).  sqair_amd/lane.py
holds all of it and says what each returns.

The stream takes over its core's handle: while it is open, every inference pass of that handle carries the state.  ``close()``
hands the handle back.

``state``: a blob of the same core and B to continue from (for example ``StreamTrainer.state``, sqair_amd/train.py, after training on
the stream): the first step then imports every row from it instead of starting fresh.  It is copied; the stream's frame count
(the default noise key) starts at 0.
"""
from __future__ import annotations

import ctypes as C

import torch

from sqair_amd import _capi
from sqair_amd.carried import CarriedState, blank_unobserved, carried, check_observed
from sqair_amd.lane import LaneAnswers, TrajScores, check_unit, field_views, is_int_in, lane_answer, zeros_of

DEFAULT_OUTPUTS = ("what", "where", "presence", "obj_id", "log_weights_per_timestep")
FORECAST_OUTPUTS = ("what", "where", "presence", "presence_prob", "presence_logit", "obj_id", "canvas", "glimpse")
# Philox step key of the default forecast noise: the top bit set, the frames consumed below it -- never a step's key (its frame index)
FORECAST_NOISE_TAG = 1 << 63


class SqairStream(object):
    def __init__(self, core, B, frames_per_step=1, outputs=DEFAULT_OUTPUTS, use_graph=True, seed=0, resample=None, ess_frac=0.5,
                 state=None, history=None, history_fields=tuple(_capi.HISTORY_FIELDS), missing=False, estimate=False,
                 estimate_iou=0.5, estimate_canvas=False, estimate_layers=False, layers_cover_min=0.5, score=False, score_iou=0.5,
                 score_truth=None, identity=False, identity_iou=0.3, identity_tracks=None, identity_max_age=10, identity_reid_dist=4.0,
                 identity_reid_what=float("inf"), identity_appearance=True, score_ids="row", score_idf=False, score_idf_ids=32,
                 score_match="greedy", identity_match="greedy", score_hota=False, score_hota_ids=32, score_hota_frames=256,
                 motion=False, motion_q=0.25, motion_r=1.0, motion_v0=16.0, motion_gate=3.0, motion_nis=False, tracklog=None,
                 tracklog_tracks=16, tracklog_truth=None):
        if core.cfg.sample_from_prior:
            raise ValueError("SqairStream: generation modes (sample_from_prior) do not carry a state across calls")
        if resample not in (None, "systematic"):
            raise ValueError("SqairStream: resample must be None or 'systematic'")
        ess_frac = float(ess_frac)
        if resample is not None and not 0.0 <= ess_frac <= 1.0:   # (NaN fails too)
            raise ValueError("SqairStream: ess_frac must lie in [0, 1]")
        la = self.lane = LaneAnswers("SqairStream", estimate, estimate_iou, estimate_canvas, estimate_layers, layers_cover_min, score,
                                     score_iou, score_truth, identity, identity_iou, identity_tracks, identity_max_age,
                                     identity_reid_dist, identity_reid_what, identity_appearance, score_ids, score_idf, score_idf_ids,
                                     score_match, identity_match, score_hota, score_hota_ids, score_hota_frames, motion, motion_q,
                                     motion_r, motion_v0, motion_gate, motion_nis, tracklog, tracklog_tracks, tracklog_truth)   # (checks only)
        self.smc = resample is not None
        self.ess_frac = ess_frac
        self.core = core
        self.B, self.K = int(B), core.K
        self.R = self.B * self.K
        self.T = int(frames_per_step)
        if self.B < 1 or self.T < 1:
            raise ValueError("SqairStream: B and frames_per_step must be >= 1")
        la.size(core)   # (the last check that needs the core's N: still before the handle is touched)
        outputs = tuple(outputs)
        if "log_weights_per_timestep" not in outputs:   # (the running log-weight sums)
            outputs = outputs + ("log_weights_per_timestep",)
        if history is not None:   # (checked before the handle is touched; the ring records these outputs of the pass)
            outputs = outputs + tuple(f for f in CarriedState.check_history(history, history_fields, "SqairStream") if f not in outputs)
        if estimate_canvas and "canvas" not in outputs:   # (mean_canvas averages the pass's canvases)
            outputs = outputs + ("canvas",)
        self.outputs = outputs
        self.use_graph = bool(use_graph)
        self.seed = int(seed)
        self.frame = 0          # frames consumed so far (host side; the rows' own counters are in the blob)
        core.bind(self.T, self.B, list(outputs))
        # the blob, the source map (host-side until a step uploads it; SMC: on the device) and the weights (sqair_amd/carried.py)
        cs = self.carried = CarriedState(core, self.B, "SqairStream", self.smc)
        if state is not None:   # hand-over: the first step continues every row of the given blob
            cs.adopt(state)
        self._graph = False
        self._tr = {}               # tracks() buffers of the LAST (lag, start, max_tracks, table, lane, lane_iou) only
        self._fc = {}               # forecast buffers of the LAST (F, outputs, summaries, samples, lane) only: workspace, noise, map, weights, outputs
        self.traj = TrajScores(core, self.B, la)   # trajectory scores by kind: accumulators and outputs of the LAST (F, G, truth_iou)
        self._smc_uniforms = None   # registered with the caller's uniforms (True) or Philox (False)
        core.stream.synchronize()
        core.check(core.lib.sqair_set_state(core.handle, cs.state.data_ptr(), cs.state.data_ptr(), cs._src.data_ptr(),
                                            cs.state.numel() * 4, self.B), "sqair_set_state")
        if self.smc:
            self._set_smc(False)
        self.missing = bool(missing)
        if self.missing:   # the device mask [T', B] the pass's kernels read: all observed until a step says otherwise
            self._observed = torch.ones((self.T, self.B), dtype=torch.int32, device=core.device)
            self._every_lane = torch.ones((self.T, self.B), dtype=torch.bool, device=core.device)   # what step() returns without a mask
            self._observed_is_ones = True
            torch.cuda.current_stream(core.device).synchronize()
            core.check(core.lib.sqair_set_observed(core.handle, self._observed.data_ptr(), self.T, self.B), "sqair_set_observed")
        la.register(core, cs.log_weight_sum, self.T, self.B)   # after SMC: the estimate's log_w must be the resampler's accumulator
        if history is not None:
            ring, nb, bits = cs.set_history(history, history_fields, self.T)
            torch.cuda.current_stream(core.device).synchronize()   # (the ring's zeros are in place before a pass pushes into it)
            core.check(core.lib.sqair_set_history(core.handle, ring.data_ptr(), nb, cs.history, bits), "sqair_set_history")
        core._graph_ready = False   # (the handle's graph is now this stream's)

    # the carried state's, read-only (_src, _armed, _src_is_identity: what the tests and tools look at)
    state, log_weight_sum, log_z, log_evidence, ess, u, resampled, _src, _armed, _src_is_identity, history, history_fields = (
        carried(n) for n in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src", "_armed",
                             "_src_is_identity", "history", "history_fields"))
    # the lane answers', likewise
    estimate, scored, identified, G, M, _est_flat, _est_views, _est, _score, _ident, _idf, _hota, _tracklog, _truth_ring = (
        lane_answer(n) for n in ("estimate", "scored", "identified", "G", "M", "flat", "views", "est", "score_buf", "ident_buf", "idf_buf",
                                 "hota_buf", "tracklog_buf", "truth_ring"))
    _traj = lane_answer("acc", of="traj")

    def _set_smc(self, uniforms):
        """Registers the SMC buffers (sqair_set_smc), the lane uniforms read from ``_uniforms`` or drawn by Philox.  The pointers
        are frozen into the captured graph: switching between the two recaptures it on the next step."""
        if self._smc_uniforms is uniforms:
            return
        smc = self.carried.smc_struct(self.ess_frac, self.seed, uniforms)
        core = self.core
        core.check(core.lib.sqair_set_smc(core.handle, C.byref(smc), self.B), "sqair_set_smc")
        self._smc_uniforms = uniforms
        self._graph = False

    # ---- source map -------------------------------------------------------------------------------------------------------
    def reset(self, lanes):
        """Lanes (sequences, in [0, B)) whose next step starts a new clip: their K particle rows start fresh, counter 0.  A scored
        stream also forgets those lanes' identities (``last_id``: a new clip has new ones); their counters stay.  A stream with
        ``identity=True`` frees those lanes' track entries (``trk_id`` = -1) and keeps their ``next_id``: an id is never reused within
        a lane.  A stream with ``score_idf=True`` first closes those lanes' clips (one solve on the device): their IDF1 figures go
        into the totals and their tables are freed -- a new clip has new truth identities.  A stream with ``score_hota=True`` closes
        their HOTA clips the same way.  A stream with ``tracklog`` empties those lanes' logs (``count`` = 0)."""
        self.carried.reset(lanes)
        self.lane.reset(sorted(set(self.carried.check_lanes(lanes))), self.carried._on_core_stream)

    def resample(self, src_rows):
        """Row r of the next step continues row src_rows[r] (-1: starts fresh); e.g. SMC resampling of the particles of each
        sequence, src[b*K + k] = b*K + k'.  Composes with a reset armed before it.  The running log-weight sums follow the rows.
        With SMC on it composes on the device with the map the last step's resampler wrote: src_new[r] = src[src_rows[r]]."""
        self.carried.resample(src_rows)

    # ---- stepping ---------------------------------------------------------------------------------------------------------
    def _check_observed(self, observed):
        """``observed`` of a step as a bool tensor [T', B] (None: every lane has its frame)."""
        return check_observed(observed, self.missing, self.T, self.B, "SqairStream", "stream")

    _blank_unobserved = staticmethod(blank_unobserved)

    def step(self, frames, noise=None, seed=None, uniforms=None, observed=None, truth=None):
        """Consumes frames [T', B, H, W] (T' = frames_per_step); returns this step's per-frame outputs {name: [T', B*K, ...]}
        (copies, valid on the current stream).  ``noise`` [T', B*K, 2, N, 4 + n_what + 1]; default: the library's generator
        keyed by (``seed`` or the stream's seed, frame index).  With SMC on, also ``ess``, ``resampled``, ``log_evidence`` [B]
        and ``ancestors`` [B*K] (the next step's source map), device copies taken before anything is read on the host;
        ``uniforms`` [B] in [0, 1): this step's systematic-resampling uniforms (default: Philox).  ``observed`` (streams with
        ``missing=True``): bool [T', B], or [B] when T' = 1, False = the lane has no frame and coasts on the prior; its frame is
        replaced by zeros, so it may hold anything, NaN included.  Default: every lane observed.  Returned among the outputs.
        Streams with ``estimate=True`` add ``lane``: the per-lane answer {name: [T', B, ...]} of this step's rows.  ``truth``
        (streams with ``score=True``): dict(box=[T', B, G, 4] (y, x, h, w) in pixels, present=[T', B, G], valid=[T', B] or None = all),
        with [B, ...] accepted when T' = 1; the step's lane answer is scored against it.  Default: nothing is scored.  Streams with
        ``tracklog_truth=G`` take it too, with or without ``score=True``, and keep it in the track log's truth ring for
        ``track_log(score=True)``; a step without it leaves its frames of the ring without truth."""
        observed = self._check_observed(observed)   # (before the core is touched)
        truth = self.lane.check_truth(truth)
        core, cs = self.core, self.carried
        frames, noise, uniforms = cs.check_inputs(self.T, frames, noise, uniforms, "stream")
        if observed is not None:
            if frames.is_cuda:   # (one upload at most: the blanking, the registered mask and the returned one share it)
                observed = observed.to(frames.device)
            frames = self._blank_unobserved(frames, observed)
        if self.smc:
            self._set_smc(uniforms is not None)
        lib = core.lib
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                cs.feed(frames, noise, uniforms, self.seed if seed is None else int(seed), self.frame)
                if self.missing:   # (a mask that lives on the device, like the frames of a resident clip, costs no upload)
                    if observed is not None:
                        observed = observed.to(core.device, non_blocking=True)
                        self._observed.copy_(observed)
                    elif not self._observed_is_ones:
                        self._observed.fill_(1)
                    self._observed_is_ones = observed is None
                self.lane.feed_truth(truth)
                if self.use_graph:
                    if not self._graph:
                        core.stream.synchronize()
                        core.check(lib.sqair_graph_capture(*core._args(0)), "sqair_graph_capture")
                        self._graph = True
                    core.check(lib.sqair_graph_launch(core.handle, core._stream()), "sqair_graph_launch")
                else:
                    core.check(lib.sqair_forward(*core._args(0)), "sqair_forward")
                out = {k: core.out[k].clone() for k in self.outputs}
                if self.missing:
                    out["observed"] = self._every_lane if observed is None else observed
                if self.estimate:
                    out["lane"] = self.lane.copy_out()
                if self.smc:   # (log_weight_sum is the resampler's accumulator)
                    out.update(ess=cs.ess.clone(), resampled=cs.resampled.clone(), log_evidence=cs.log_evidence.clone(),
                               ancestors=cs._src.clone())
                else:
                    cs.log_weight_sum += out["log_weights_per_timestep"].sum(0)
            core._join_out()
        self.frame += self.T
        return out

    # ---- scoring ----------------------------------------------------------------------------------------------------------
    def score(self, reset=False):
        """The score so far (include/sqair_hip.h: sqair_set_score): per lane the int64 counters ``frames``, ``frames_invalid``,
        ``truth``, ``tp``, ``fn``, ``fp``, ``idsw``, ``count_hit``, ``count_abs_err`` [B] and the fp64 ``iou_sum`` [B] (host tensors), and
        pooled over the lanes ``mota`` = 1 - (fn + fp + idsw) / truth, ``motp`` = iou_sum / tp and ``count_accuracy`` = count_hit /
        frames, each NaN where its denominator is 0.  ``reset``: the counters and ``iou_sum`` start again from zero afterwards; the
        identity memory stays (``reset(lanes)`` clears that)."""
        return self.lane.score(reset)

    def idf_score(self, reset=False):
        """The identity measures so far (include/sqair_hip.h: sqair_set_idf): one solve on the device, nothing closed.  Per lane, the
        totals over the closed clips plus the open clip, the int64 figures ``clips``, ``frames``, ``trajectories``, ``idtp``, ``idfn``,
        ``idfp``, ``mt``, ``pt``, ``ml``, ``frag_per_lane``, ``ids``, ``overflow_ids`` [B] (host tensors);
        ``assign`` [B, G] int32, the id word assigned to each truth of the open clip (-1: none; optimal assignments tie); pooled over the
        lanes ``idf1`` = 2 idtp / (2 idtp + idfp + idfn), ``idp`` = idtp / (idtp + idfp), ``idr`` = idtp / (idtp + idfn), ``mt_rate`` =
        mt / trajectories, ``ml_rate`` = ml / trajectories, each NaN where its denominator is 0, ``frag`` the fragmentations and
        ``exact``: no frame held an object without a column (``overflow_ids`` == 0: more than ``score_idf_ids`` ids in a clip, a
        negative id word).  ``reset``: the totals start again from zero and every table is freed afterwards."""
        return self.lane.idf_score(reset)

    def hota_score(self, reset=False):
        """HOTA so far (include/sqair_hip.h: sqair_set_hota): one solve on the device, nothing closed.  Per lane, the totals over the
        closed clips plus the open clip: ``tp``, ``fn``, ``fp``, ``loc`` [B, 19] int64 and ``ass_sum``, ``assre_sum``, ``asspr_sum`` [B, 19] float64
        per threshold alpha = 0.05 .. 0.95, ``clips``, ``frames``, ``dropped_frames``, ``overflow_ids`` [B] (host tensors).  Pooled over
        the lanes -- counts add, AssA is weighted by TP, as TrackEval combines sequences -- and, in ``lanes`` [B], for each lane alone:
        ``hota_alpha``, ``deta_alpha``, ``assa_alpha`` [19] with DetA = tp / (tp + fn + fp), AssA = ass_sum / tp and HOTA_alpha =
        sqrt(DetA AssA); their means over the thresholds ``hota``, ``deta``, ``assa``, ``detre``, ``detpr``, ``assre``, ``asspr``,
        ``loca``; ``hota0`` and ``loca0`` at alpha = 0.05; each NaN where a denominator is 0.  ``exact``: no frame was dropped (a clip
        longer than ``score_hota_frames``) and no object was without a column (more than ``score_hota_ids`` ids in a clip, a negative
        id word).  ``reset``: the totals start again from zero and every log is freed afterwards."""
        return self.lane.hota_score(reset)

    # ---- lane identities --------------------------------------------------------------------------------------------------
    def identities(self):
        """The identities so far (include/sqair_hip.h: sqair_set_identity): per lane the int64 counters ``frames``, ``frames_invalid``,
        ``objects``, ``kept``, ``bridged``, ``reidentified``, ``born``, ``ended`` [B] and ``next_id`` [B]; pooled over the lanes
        ``bridged_rate`` = bridged / objects and ``reidentified_rate`` = reidentified / objects (NaN without objects); and the track
        table ``trk_id``, ``trk_age``, ``trk_len`` [B, M] and ``trk_box`` [B, M, 4] (host tensors): the entries with ``trk_id`` >= 0 and
        ``trk_age`` > 0 are the tracks remembered but currently unseen.  With ``motion=True`` also the filter's state (sqair_set_motion):
        ``trk_centre``, ``trk_vel``, ``trk_sigma`` [B, M, 2] and ``trk_pred_box`` [B, M, 4], the coasted box of every live track."""
        return self.lane.identities()

    def track_log(self, lag=None, q=None, r=None, v0=None, score=False, score_iou=0.5, score_match="greedy", stitch=False,
                  stitch_gate=3.5, stitch_max_gap=None):
        """The trajectories of the last ``lag`` logged frames (default: all ``tracklog`` = L of them) per ``lane_id`` (include/sqair_hip.h:
        sqair_set_tracklog, sqair_lane_tracklog_smooth): one launch on the device.  C = ``tracklog_tracks`` columns per lane.
        ``track_id`` [B, C] int32, the C largest ids of the window ascending, -1 = padding; ``n_tracks`` [B], the distinct ids of the
        window, kept or not; ``len0`` [B, C], the ``track_len`` at the id's first frame in the window (1: born inside it);
        ``frame_index`` [lag, B] int64, the frames' absolute numbers since the lane's last reset, -1 before its first; ``state``
        [lag, B, C] int32 -- 0 outside the track's span, 1 seen, 2 a gap inside the span (the model's prediction stands), 3 a
        non-finite frame inside the span (nothing steps) --; ``size`` [lag, B, C, 2], (h, w) as last seen.  ``smooth`` and
        ``filtered``: dicts of ``centre``, ``velocity``, ``sigma`` [lag, B, C, 2] = (y, x) and ``box`` [lag, B, C, 4] = (y, x, h, w), the
        Rauch-Tung-Striebel smoothed and the causal estimate of a constant-velocity filter started at the track's first frame in
        the window; 0 where ``state`` is 0 or 3.  ``q``, ``r``, ``v0``: the filter's scalars, default the stream's ``motion_q``,
        ``motion_r``, ``motion_v0`` (set or not: the log does not need ``motion=True``).  Host tensors.
        ``score=True`` (a stream with ``tracklog_truth=G``) scores the table against the truth the steps were given, one more launch
        directly behind the solve (include/sqair_hip.h: sqair_lane_tracklog_score, which states the semantics), and adds ``score``:
        per view -- ``"filtered"`` (what a causal tracker reported), ``"smooth"``, ``"filtered_filled"`` and ``"smooth_filled"`` (the
        gaps filled by the model: what ``mot_rows`` exports) -- the per-lane counters ``frames``, ``frames_invalid``, ``truth``, ``tp``,
        ``fn``, ``fp``, ``idsw``, ``gap_tp``, ``gap_fp``, ``nees_n``, ``gap_nees_n``, ``idtp``, ``idfn``, ``idfp`` [B] int64 and sums
        ``iou_sum``, ``err_sum``, ``nees_sum``, ``gap_err_sum``, ``gap_nees_sum`` [B] float64, ``assign`` [B, G] (the column the window's
        identity assignment gives each truth, -1 none), ``match`` and ``match_iou`` [lag, B, G] (the column matched per frame), and pooled
        over the lanes ``mota``, ``motp``, ``idf1``, ``idp``, ``idr``, ``mean_err`` (pixels between the centres of a matched pair), ``nees``
        (its normalised square: 2 for an honest ``sigma``), ``gap_err``, ``gap_nees`` and ``gap_precision`` = gap_tp / (gap_tp + gap_fp)
        over the filled gaps; NaN where a denominator is 0.  ``score_iou``: the IoU a pair needs; ``score_match``: per-frame matching
        as keep + "greedy" or keep + "optimal".  The figures are those of this window alone: windows overlap, nothing accumulates.
        Without ``score`` nothing more is launched.
        ``stitch=True`` joins the fragments of a track with hindsight, one more launch directly behind the solve on its device tensors
        (include/sqair_hip.h: sqair_lane_tracklog_stitch, which states the semantics): a column that ended is linked to a column born
        later (``len0`` == 1) across at most ``stitch_max_gap`` counting frames (default ``lag``) when the old one's coasted state and
        the new one's smoothed state at birth lie within ``stitch_gate`` sigmas (four degrees of freedom), the links are chosen one
        to one on the device, and the joined columns are filtered and smoothed again.  The result gains ``stitched``: the same keys
        as the plain result for the stitched table -- ``mot_rows(res["stitched"], lane)`` works unchanged -- and ``links``: ``next``
        [B, C] (the successor's column in the plain table, -1 none), ``d2`` (0 without a link), ``gap`` (-1 without), ``root`` [B, C]
        (the stitched column a plain column went to) and ``n_links`` [B].  With ``score=True`` as well the scorer runs a second time,
        on the stitched table, into ``stitched["score"]``.  Without ``stitch`` nothing more is launched and the result is unchanged."""
        return self.lane.track_log(lag, q, r, v0, score, score_iou, score_match, stitch, stitch_gate, stitch_max_gap)

    def track_log_fit(self, lag=None, q_grid=None, r_grid=None, v0=None, burn=2, innov=False):
        """Motion calibration: the maximum-likelihood ``q`` and ``r`` of the motion model on a grid, from the last ``lag`` logged frames
        and without truth (include/sqair_hip.h: sqair_lane_tracklog_fit, which states the semantics): the solve, then one more launch
        on the solve's device tensors.  Every track of the window is filtered again under every (q, r) of ``q_grid`` x ``r_grid`` (1 to
        16 values each, finite and > 0; default the stream's ``motion_q`` * 4^k and ``motion_r`` * 4^k for k = -4..3, so that the
        current scalars are node (4, 4)), conditioned on the associations the log recorded; the innovations y and their variances S
        of every later sighting but a column's first ``burn`` give the sums of -log p = 1/2 sum (ln 2 pi S + y^2 / S).  ``v0``: the
        newborn's velocity variance, default the stream's ``motion_v0`` (it is not fitted).  Returns what ``lane.track_log_fit`` forms
        (sqair_amd/lane.py): ``q``, ``r`` and ``node``, the grid node of minimal pooled ``nll``; ``at_edge``, whether it lies on the
        grid's border (fit again with a grid moved there); per node [Q, R] ``nll``, ``mean_nis`` (1 for an honest filter: the
        truth-free counterpart of the score's ``nees``), ``gap_mean_nis`` (the same over the first sightings behind a gap), ``n``,
        ``n_gap``, ``skipped`` (innovations with a non-finite or non-positive term); the same per lane under ``lane_*``, and ``lane_q``,
        ``lane_r`` [B].  ``innov=True`` adds ``innov`` [lag, B, C, 2, 2], (y, S) of node (0, 0).  Nothing of the stream changes: apply a
        fit with ``set_motion``.  Host tensors; the figures are those of this window alone."""
        return self.lane.track_log_fit(lag, q_grid, r_grid, v0, burn, innov)

    def set_motion(self, q=None, r=None, v0=None, gate=None):
        """Replaces the motion model's scalars (None: kept), each finite and > 0 as the constructor checks ``motion_q``, ``motion_r``,
        ``motion_v0`` and ``motion_gate``: the defaults of ``track_log()`` and ``track_log_fit()`` follow.  On a stream with
        ``motion=True`` the motion is also registered again with the same buffers (sqair_set_motion) -- the tracks' filter states
        ``trk_kf`` are kept -- and a captured graph is recaptured on the next step; on other streams only the defaults change."""
        if self.lane.set_motion(q, r, v0, gate):
            self._graph = False

    # ---- trajectory scoring ------------------------------------------------------------------------------------------------
    def _check_traj_truth(self, fn, truth, lane, F, default_anchor, link_ids, truth_iou, link_match="greedy"):
        return self.traj.check_truth(fn, truth, lane, F, default_anchor, link_ids, truth_iou, link_match)

    def trajectory_score(self, kind, reset=False):
        """The trajectory score so far of ``kind`` = "forecast" or "tracks" (include/sqair_hip.h: sqair_lane_traj_score): what the
        calls with ``truth`` have accumulated.  Per (frame or horizon f, lane) the int64 counters ``frames``, ``pairs``, ``hits``,
        ``lost``, ``gone``, ``count_hit``, ``count_abs_err`` [F, B] and the fp64 ``iou_sum``, ``centre_err_sum``, ``brier_sum`` [F, B]; per
        lane ``calls``, ``calls_invalid``, ``anchor_truth``, ``linked`` [B] (host tensors).  Pooled over the lanes, per f, NaN where the
        denominator is 0: ``ade`` = centre_err_sum / pairs (``fde`` = its last entry), ``mean_iou`` = iou_sum / pairs, ``hit_rate`` =
        hits / (pairs + lost), ``brier`` = brier_sum / (pairs + lost + gone), ``count_accuracy`` = count_hit / frames [F] (float64), and
        ``link_rate`` = linked / anchor_truth.  The accumulators belong to (kind, F, G, truth_iou, link_match): a call with truth of another F, G,
        threshold or matching starts fresh ones and drops the old.  ``reset``: they start again from zero afterwards."""
        return self.traj.read(kind, reset)

    # ---- forecasting ------------------------------------------------------------------------------------------------------
    def forecast(self, F, noise=None, seed=None, outputs=FORECAST_OUTPUTS, summaries=True, samples=1, lane=False, lane_iou=0.5,
                 truth=None, link_ids=False, truth_iou=0.5, link_match="greedy"):
        """Rolls the generative prior F frames forward from the rows the next ``step()`` would start from -- the state blob through
        the pending source map (a reset or resample armed since the last step, else identity; with SMC the map the resampler
        wrote) -- and returns {name: [F, B*K, ...]} for ``outputs`` (of FORECAST_OUTPUTS).  With ``summaries`` also the lanes'
        predictive ``mean_canvas`` [F, B, H, W] and ``expected_count`` [F, B] under the particle weights, and those normalised
        ``weights`` [B, K] (softmax of each lane's running log-weight sums, gathered through the same map).  ``noise``
        [F, B*K, 2, N, 4 + n_what + 1] (slot s = 0 is read); default: the library's Philox keyed by (``seed`` or the stream's
        seed, FORECAST_NOISE_TAG | frames consumed), apart from every step's draws.  Copies, valid on the current stream.  Nothing
        the steps read is written.  The stream keeps one set of forecast buffers (workspace, noise, outputs), for the last
        (F, outputs, summaries, samples, lane) asked for: repeating a shape reuses them, another shape frees them and allocates its own.
        ``samples`` = S rolls every particle row forward S times in the one call (include/sqair_hip.h: sqair_forecast_fan): the per-row
        results become [F, B*K*S, ...], rollout s of row r at r*S + s (``noise`` likewise), each weighing w_k / S in the summaries.
        ``lane=True`` adds ``lane``: one predictive answer per object of each lane from its K*S rollouts, {name: tensor} for
        ``best_row`` [B], ``weights`` [B, K], ``start_where`` / ``start_presence`` / ``start_obj_id`` [B*K, N, .] (the rows the rollouts
        start from), the best start row's objects ``obj_id``, ``presence`` [B, N] and ``box0`` [B, N, 4] (y, x, h, w in pixels),
        ``support`` [B, N], and per horizon ``alive`` [F, B, N] (the weight of the rollouts in which the object still lives),
        ``box_mean`` / ``box_std`` [F, B, N, 4] over those rollouts (NaN where none is left) and ``count_prob`` [F, B, N + 1];
        ``lane_iou``: the association threshold on the start rows, as a stream's ``estimate_iou``.
        ``truth`` (with ``lane=True``) scores the lane forecast against ground-truth boxes on the device, one more launch after the
        forecast's (include/sqair_hip.h: sqair_lane_traj_score, which states the semantics): dict(box=[F, B, G, 4] (y, x, h, w) in
        pixels, present=[F, B, G], valid=[F, B] or None = all -- the truth at the forecast's frames --, anchor_box=[B, G, 4],
        anchor_present=[B, G], anchor_valid=[B] or None = all -- the truth at the last stepped frame, required: truth and lane objects
        are linked there, by IoU >= ``truth_iou``); G in [1, 16] comes from the shapes, tensors already on the device are used where
        they are.  ``res["lane"]["score"]`` holds ``link``, ``link_iou`` [B, G], ``state``, ``p_alive``, ``pair_iou``, ``centre_err`` [F, B, G]
        and ``count_map`` [F, B]; ``trajectory_score("forecast")`` reads what the calls have accumulated.  ``link_ids=True`` (a stream
        with ``score=True`` and the same G) keeps each truth with the identity the stream's score last matched it with;
        ``link_match="optimal"`` links by keep + optimal where the default is keep + greedy (sqair_set_lane_match).  Without
        ``truth`` nothing is launched, and with it every other output is unchanged bit for bit."""
        F, S, lane, lane_iou = int(F), int(samples), bool(lane), float(lane_iou)
        if F < 1:
            raise ValueError("SqairStream.forecast: F must be >= 1")
        if S < 1 or self.K * S > _capi.FORECAST_FAN_MAX:
            raise ValueError("SqairStream.forecast: samples must be >= 1 with K * samples <= {}".format(_capi.FORECAST_FAN_MAX))
        if lane:
            check_unit("SqairStream.forecast: ", "lane_iou", lane_iou)
        outputs = tuple(outputs)
        bad = [n for n in outputs if n not in FORECAST_OUTPUTS]
        if bad:
            raise ValueError("SqairStream.forecast: unknown outputs {} (choose from {})".format(bad, FORECAST_OUTPUTS))
        truth = self._check_traj_truth("SqairStream.forecast: ", truth, lane, F, False, link_ids, truth_iou, link_match)
        core, cs = self.core, self.carried
        lib, dev = core.lib, core.device
        R, N, nzw = self.R * S, core.N, core.nzw
        if noise is not None:
            noise = torch.as_tensor(noise, dtype=torch.float32)
            if noise.numel() != F * R * 2 * N * nzw:
                raise ValueError("SqairStream.forecast: noise of shape {} given, [{}, {}, 2, {}, {}] expected".format(
                    tuple(noise.shape), F, R, N, nzw))
        key = (F, outputs, bool(summaries), S, lane)
        with torch.cuda.device(dev):
            core._join_in()
            with core.on_stream():
                fc = self._fc.get(key)
                if fc is None:   # (another shape: the previous buffers are released first -- a growing horizon does not pile up)
                    self._fc.clear()
                    fc = self._forecast_buffers(F, outputs, summaries, S, lane)
                    self._fc[key] = fc
                if noise is not None:
                    fc["noise"].copy_(noise.reshape(fc["noise"].shape), non_blocking=True)
                else:
                    core.check(lib.sqair_fill_noise(core.handle, fc["noise"].data_ptr(), F, self.B * S, self.B * S, 0,
                                                    (self.seed if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF,
                                                    FORECAST_NOISE_TAG | self.frame, core._stream()), "sqair_fill_noise")
                src, lw = cs.next_rows(fc["src"], fc["log_w"])   # (the map and the weights of the rows the next step starts from)
                out = fc["out"]
                c_out = _capi.SqairForecastOutputs(**{n: t.data_ptr() for n, t in out.items()})
                if summaries or lane:
                    c_out.log_w = lw.data_ptr()
                if S == 1 and not lane:
                    core.check(lib.sqair_forecast(core.handle, core.flat.data_ptr(), core.packed.data_ptr(), fc["noise"].data_ptr(), F,
                                                  self.B, src.data_ptr(), C.byref(c_out), fc["ws"].data_ptr(), fc["ws"].numel() * 4,
                                                  core._stream()), "sqair_forecast")
                else:
                    c_lane = None
                    if lane:
                        c_lane = C.byref(_capi.SqairForecastLane(iou_min=lane_iou, **{n: t.data_ptr() for n, t in fc["lane"].items()}))
                    core.check(lib.sqair_forecast_fan(core.handle, core.flat.data_ptr(), core.packed.data_ptr(), fc["noise"].data_ptr(),
                                                      F, self.B, S, src.data_ptr(), C.byref(c_out), c_lane, fc["ws"].data_ptr(),
                                                      fc["ws"].numel() * 4, core._stream()), "sqair_forecast_fan")
                res = {k: v.clone() for k, v in out.items()}
                score = None if truth is None else self.traj.launch("forecast", fc["lane"], F, truth, link_ids, link_match)
                if lane:   # (views of one allocation: one copy, not one per field)
                    res["lane"] = fc["lane_views"](fc["lane_flat"].clone())
                    if score is not None:
                        res["lane"]["score"] = score
                if summaries:
                    res["weights"] = torch.softmax(lw.reshape(self.B, self.K), -1)
            core._join_out()
        return res

    def _forecast_buffers(self, F, outputs, summaries, S=1, lane=False):
        core = self.core
        R, N, B = self.R * S, core.N, self.B
        shapes = dict(what=(F, R, N, core.nw), where=(F, R, N, 4), presence=(F, R, N), presence_prob=(F, R, N),
                      presence_logit=(F, R, N), obj_id=(F, R, N), canvas=(F, R, core.H, core.W),
                      glimpse=(F, R, N, core.G, core.G))
        if summaries:
            shapes.update(mean_canvas=(F, B, core.H, core.W), expected_count=(F, B))
            outputs = outputs + ("mean_canvas", "expected_count")
        z = lambda shp, dt=torch.float32: torch.zeros(shp, dtype=dt, device=core.device)
        if S == 1 and not lane:
            nb = core.lib.sqair_forecast_workspace_bytes(core.handle, F, B)
        else:
            nb = core.lib.sqair_forecast_fan_workspace_bytes(core.handle, F, B, S)
        if nb < 0:
            raise RuntimeError("sqair_forecast_workspace_bytes failed")
        fc = dict(ws=z(nb // 4), noise=z((F, R, 2, N, core.nzw)), src=z(self.R, torch.int32), log_w=z(self.R),
                  out=zeros_of("SqairForecastOutputs", {n: shapes[n] for n in outputs}, core.device))
        if lane:   # the fields of SqairForecastLane as views of ONE allocation
            fc["lane_flat"], fc["lane_views"] = field_views(_capi.forecast_lane_shapes(F, B, self.K, N), _capi.FORECAST_LANE_INT_FIELDS,
                                                             core.device)
            fc["lane"] = fc["lane_views"](fc["lane_flat"])
        return fc

    # ---- track history ----------------------------------------------------------------------------------------------------
    def tracks(self, lag=None, start="next", max_tracks=None, table=True, lane=False, lane_iou=0.5, truth=None, link_ids=False,
               truth_iou=0.5, link_match="greedy"):
        """Traces every particle row's ancestral path back over the last ``lag`` steps (default: all ``history`` kept) on the
        device: frames oldest -> newest, F = lag * frames_per_step.  ``start="next"``: from the rows the next ``step()`` would
        start from (the pending source map; with SMC the map the resampler wrote: the equally weighted surviving set), as
        ``forecast`` does; ``"last"``: from the rows of the last step's outputs.  Returns ``where`` [F, B*K, N, 4], ``presence``,
        ``obj_id`` [F, B*K, N], with the fields kept ``what`` [F, B*K, N, n_what] and ``log_w`` [F, B*K] -- the values stored at the
        ancestor's row, zero where the path has ended (a fresh row, a -1 start, a step not kept any more) --, ``valid`` and
        ``frame_index`` [F, B*K] (the row's frame counter, -1 where invalid), ``ancestor_row`` [lag, B*K] and ``unique_ancestors``
        [lag, B]: the distinct ancestors among a lane's K paths (how far back more than one hypothesis survives).  With ``table``
        the tracks by object id: ``track_id`` [B*K, M] (ascending, -1 padded; M = ``max_tracks``, default 2 N), ``n_tracks`` [B*K]
        (the true count; above M: truncated), ``track_present`` [F, B*K, M], ``track_where`` [F, B*K, M, 4].  With
        ``start="next"`` also the particles' ``weights`` [B, K] (as ``forecast`` forms them) and ``best_row`` [B], the first row of
        maximal weight per lane.  Copies, valid on the current stream; nothing the steps read is written.  One set of buffers is
        kept, for the last (lag, start, max_tracks, table, lane, lane_iou) asked for.
        ``lane=True`` (needs ``start="next"``) adds ``lane``: one smoothed trajectory per object of each lane from its K traced paths
        (include/sqair_hip.h: sqair_history_trace_lane), the backward-looking twin of ``forecast(lane=True)``, weighed by the weights
        ``forecast`` would use: ``best_row`` [B], ``weights`` [B, K], the objects of the best row's newest frame ``obj_id``,
        ``presence`` [B, N], ``box0`` [B, N, 4] and ``support`` [B, N] -- the same objects in the same order as the lane forecast taken
        between the same two steps --, ``first_frame`` [B, N] (the oldest frame the best row's own path holds the object from), and
        per traced frame ``alive`` [F, B, N] (the weight of the particles whose path holds the object there), ``box_mean`` /
        ``box_std`` [F, B, N, 4] over them (NaN where none does), ``count_prob`` [F, B, N + 1] and ``valid_mass`` [F, B] (the weight of
        the paths that reach back to the frame: ``count_prob`` sums to it, not to 1); ``lane_iou``: the association threshold.
        ``truth``, ``link_ids``, ``truth_iou`` (with ``lane=True``): the lane tracks scored against ground-truth boxes as ``forecast``'s
        lane answer is, ``truth["box"]`` [F, B, G, 4] and ``truth["present"]`` [F, B, G] being the truth at the traced frames; the anchor
        defaults to their frame F - 1 (and ``anchor_valid`` to ``valid[F - 1]``), the last stepped frame; frames no path reaches back to
        (``valid_mass`` 0) are not scored.  ``res["lane"]["score"]`` and ``trajectory_score("tracks")`` as there."""
        core, cs = self.core, self.carried
        if cs.ring is None:
            raise ValueError("SqairStream.tracks: the stream keeps no history (SqairStream(..., history=L))")
        lag = cs.history if lag is None else lag
        if not is_int_in(lag, 1, cs.history):
            raise ValueError("SqairStream.tracks: lag must be an integer in [1, history = {}]".format(cs.history))
        if start not in ("next", "last"):
            raise ValueError("SqairStream.tracks: start must be 'next' or 'last'")
        M = 2 * core.N if max_tracks is None else max_tracks
        if table and not is_int_in(M, 1, 1024):
            raise ValueError("SqairStream.tracks: max_tracks must be an integer in [1, 1024]")
        lane, lane_iou = bool(lane), float(lane_iou)
        if lane and start != "next":
            raise ValueError("SqairStream.tracks: lane=True requires start='next': the lane answer is weighed by the weights of the rows "
                             "the next step starts from, as forecast()'s is")
        if lane:
            check_unit("SqairStream.tracks: ", "lane_iou", lane_iou)
        lag, M = int(lag), int(M)
        truth = self._check_traj_truth("SqairStream.tracks: ", truth, lane, lag * self.T, True, link_ids, truth_iou, link_match)
        key = (lag, start, M if table else None, bool(table), lane, lane_iou if lane else None)
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                tr = self._tr.get(key)
                if tr is None:
                    self._tr.clear()
                    tr = self._tr[key] = self._track_buffers(lag, M, table, lane)
                src = None
                if start == "next":
                    src, lw = cs.next_rows(tr["src"], tr["log_w"])
                c_out = _capi.SqairTraceOutputs(T=self.T, max_tracks=M, **{n: t.data_ptr() for n, t in tr["out"].items()})
                if lane:
                    c_lane = _capi.SqairTraceLane(iou_min=lane_iou, **{n: t.data_ptr() for n, t in tr["lane"].items()})
                    core.check(core.lib.sqair_history_trace_lane(core.handle, cs.ring.data_ptr(), src.data_ptr(), lag, C.byref(c_out),
                                                                 lw.data_ptr(), C.byref(c_lane), tr["lane_scratch"].data_ptr(),
                                                                 tr["lane_scratch"].numel() * 4, core._stream()),
                               "sqair_history_trace_lane")
                else:
                    core.check(core.lib.sqair_history_trace(core.handle, cs.ring.data_ptr(), None if src is None else src.data_ptr(),
                                                            lag, C.byref(c_out), core._stream()), "sqair_history_trace")
                res = {k: v.clone() for k, v in tr["out"].items()}
                score = None if truth is None else self.traj.launch("tracks", tr["lane"], lag * self.T, truth, link_ids, link_match)
                if lane:   # (views of one allocation: one copy, not one per field)
                    res["lane"] = tr["lane_views"](tr["lane_flat"].clone())
                    if score is not None:
                        res["lane"]["score"] = score
                if start == "next":
                    w = res["weights"] = torch.softmax(lw.reshape(self.B, self.K), -1)
                    k = torch.arange(self.K, device=core.device)
                    first = torch.where(w == w.max(-1, keepdim=True).values, k, self.K).min(-1).values % self.K
                    res["best_row"] = (first + torch.arange(self.B, device=core.device) * self.K).to(torch.int32)
            core._join_out()
        return res

    def _track_buffers(self, lag, M, table, lane=False):
        core = self.core
        R, N, B, F = self.R, core.N, self.B, lag * self.T
        shapes = dict(where=(F, R, N, 4), presence=(F, R, N), obj_id=(F, R, N), valid=(F, R), frame_index=(F, R), ancestor_row=(lag, R),
                      unique_ancestors=(lag, B))
        if "what" in self.history_fields:
            shapes["what"] = (F, R, N, core.nw)
        if "log_weights_per_timestep" in self.history_fields:
            shapes["log_w"] = (F, R)
        if table:
            shapes.update(track_id=(R, M), n_tracks=(R,), track_present=(F, R, M), track_where=(F, R, M, 4))
        z = lambda shp, dt=torch.float32: torch.zeros(shp, dtype=dt, device=core.device)
        tr = dict(src=z(R, torch.int32), log_w=z(R), out=zeros_of("SqairTraceOutputs", shapes, core.device))
        if lane:   # the fields of SqairTraceLane as views of ONE allocation, and the scratch between the two lane launches
            tr["lane_flat"], tr["lane_views"] = field_views(_capi.track_lane_shapes(F, B, self.K, N), _capi.TRACK_LANE_INT_FIELDS,
                                                             core.device)
            tr["lane"] = tr["lane_views"](tr["lane_flat"])
            nb = core.lib.sqair_trace_lane_scratch_bytes(core.handle, B, self.K)
            if nb < 0:
                raise RuntimeError("sqair_trace_lane_scratch_bytes failed")
            tr["lane_scratch"] = z(nb // 4)
        return tr

    def close(self):
        """Switches the estimate, the history and the carried state off on the core's handle (its passes start from the initial
        state again)."""
        core = self.core
        if core.handle:
            core.stream.synchronize()
            core.check(core.lib.sqair_set_estimate(core.handle, None, 0, 0), "sqair_set_estimate")
            core.check(core.lib.sqair_set_history(core.handle, None, 0, 0, 0), "sqair_set_history")
            core.check(core.lib.sqair_set_state(core.handle, None, None, None, 0, 0), "sqair_set_state")
            core.check(core.lib.sqair_set_lane_match(core.handle, 0, 0, 0), "sqair_set_lane_match")   # (a plain setting: nothing above resets it)
            core._graph_ready = False
