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

With ``estimate=True`` a step also returns ``out["lane"]``: one answer per lane and frame from the K particles, formed by one more
kernel of the pass before the resampler zeroes the weights (include/sqair_hip.h: sqair_set_estimate, which states the semantics):
the normalised ``weights`` [T', B, K] and ``ess`` [T', B] of the step's own rows, ``best_row``, the count posterior ``count_prob``
[T', B, N + 1] with ``expected_count`` and ``map_count``, the best row's objects (``presence``, ``obj_id``, ``where``, ``what``) with
their ``box`` [T', B, N, 4] = (y, x, h, w) in pixels, and per object the ``support`` -- the weight of the particles that hold a box
of IoU >= ``estimate_iou`` with it -- and their weighted mean box ``box_mean``; with ``estimate_canvas`` the posterior mean
reconstruction ``mean_canvas`` [T', B, H, W].

With ``estimate_layers=True`` (a stream with ``estimate=True``) ``out["lane"]`` also says which pixels each object of the lane
occupies, by one more kernel of the pass directly after the estimate's (include/sqair_hip.h: sqair_set_layers, which states the
semantics): ``match`` [T', B, K, N] -- the slot of particle k associated with object j, -1 where it does not agree -- and, over the
particles that agree, the weighted mean of what the decoder drew for the object: its appearance ``layer`` and its coverage ``cover``
[T', B, N, H, W]; ``owner`` [T', B, H, W] is the object of largest coverage at a pixel, -1 (background) below ``layers_cover_min``.

With ``score=True`` (a stream with ``estimate=True``) the lane answer is scored against ground-truth boxes inside the pass, by one more
kernel after the estimate's and the layers' (include/sqair_hip.h: sqair_set_score, which states the semantics): a step takes
``truth=dict(box=[T', B, G, 4], present=[T', B, G], valid=[T', B] or None)`` -- (y, x, h, w) in pixels as ``make_sequences``'s
``coords``, G = ``score_truth`` slots per lane, an object keeping its slot for its life -- copied into stream-owned device buffers
the way ``observed`` is; a step without ``truth`` scores nothing.  Present truths and present lane objects of IoU >= ``score_iou``
are matched one to one (an object's last identity first, then greedily by IoU) and the CLEAR-MOT events counted on the device:
``out["lane"]`` gains ``truth_match``, ``match_iou`` [T', B, G] and ``tp``, ``fn``, ``fp``, ``idsw`` [T', B] (-1 where nothing was scored),
and ``score()`` reads the accumulators: per lane ``frames``, ``frames_invalid``, ``truth``, ``tp``, ``fn``, ``fp``, ``idsw``,
``count_hit``, ``count_abs_err`` and ``iou_sum``, pooled ``mota``, ``motp`` and ``count_accuracy``.  ``reset(lanes)`` also forgets
those lanes' identities (a new clip has new ones) and keeps their counters.

With ``identity=True`` (a stream with ``estimate=True``) every object of the lane answer carries a track id that stays on it for as
long as the tracker can tell it is the same object, formed by one more kernel of the pass after the estimate's and the layers' and
before the score's (include/sqair_hip.h: sqair_set_identity, which states the semantics).  ``obj_id`` is the best row's per-row
counter and changes when the best row switches; ``lane_id`` does not: a table of ``identity_tracks`` (default min(16, 2 N)) tracks
per lane is kept on the device, and each frame's objects are linked to it by position (IoU >= ``identity_iou``, the same obj_id
first), then -- ``identity_reid_dist`` > 0 -- an object that was dropped for up to ``identity_max_age`` frames is re-identified when
its centre lies within ``identity_reid_dist`` pixels per frame unseen and, with ``identity_appearance``, its ``what`` within
``identity_reid_what`` of the track's (the nearest appearance wins), else it is born under a fresh id.  ``out["lane"]`` gains
``lane_id``, ``id_how`` (0 born, 1 kept, 2 bridged -- the obj_id changed under it --, 3 re-identified) and ``track_len`` [T', B, N]
int32, -1 where the slot is absent; ``identities()`` reads the counters and the table.  ``reset(lanes)`` frees those lanes' tracks;
ids are never reused within a lane.  ``score_ids="lane"`` (with ``score=True``) makes the score count its identity switches on
``lane_id`` instead of ``obj_id``.

``forecast(..., lane=True, truth=...)`` and ``tracks(..., lane=True, truth=...)`` score the two answers that reach over time -- the
lane forecast and the lane tracks -- against the truth's trajectories with one more launch after the call's own (include/sqair_hip.h:
sqair_lane_traj_score, which states the semantics): truth and lane objects are linked once, at the last stepped frame, and every
horizon or traced frame then gives displacement error, IoU, the Brier term of ``alive / support`` as a survival probability and the
count's hit, accumulated on the device per (frame, lane); ``trajectory_score(kind)`` reads the sums and pools them into curves over
the horizon (``ade``, ``fde``, ``mean_iou``, ``hit_rate``, ``brier``, ``count_accuracy``) without a lane table ever visiting the host.

The stream takes over its core's handle: while it is open, every inference pass of that handle carries the state.  ``close()``
hands the handle back.

``state``: a blob of the same core and B to continue from (for example ``StreamTrainer.state``, sqair_amd/train.py, after training on
the stream): the first step then imports every row from it instead of starting fresh.  It is copied; the stream's frame count
(the default noise key) starts at 0.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from sqair_amd import _capi
from sqair_amd.carried import CarriedState, blank_unobserved, carried, check_observed

DEFAULT_OUTPUTS = ("what", "where", "presence", "obj_id", "log_weights_per_timestep")
FORECAST_OUTPUTS = ("what", "where", "presence", "presence_prob", "presence_logit", "obj_id", "canvas", "glimpse")
# Philox step key of the default forecast noise: the top bit set, the frames consumed below it -- never a step's key (its frame index)
FORECAST_NOISE_TAG = 1 << 63


def _field_views(shapes, int_fields, device):
    """The fields {name: shape} as views of ONE float32 allocation, each 16-byte aligned (``int_fields``: viewed as int32), so that
    they are copied out with one launch instead of one per field.  Returns (flat, views): views(flat or a clone of it) -> {name: view}."""
    sizes = {n: int(np.prod(shp)) for n, shp in shapes.items()}
    offs = dict(zip(sizes, np.cumsum([0] + [(s + 3) // 4 * 4 for s in sizes.values()]).tolist()))
    flat = torch.zeros(offs[list(sizes)[-1]] + sizes[list(sizes)[-1]], dtype=torch.float32, device=device)
    return flat, lambda flat: {n: (flat[offs[n]:offs[n] + sizes[n]].view(torch.int32) if n in int_fields
                                   else flat[offs[n]:offs[n] + sizes[n]]).view(shapes[n]) for n in shapes}


class SqairStream(object):
    def __init__(self, core, B, frames_per_step=1, outputs=DEFAULT_OUTPUTS, use_graph=True, seed=0, resample=None, ess_frac=0.5,
                 state=None, history=None, history_fields=tuple(_capi.HISTORY_FIELDS), missing=False, estimate=False,
                 estimate_iou=0.5, estimate_canvas=False, estimate_layers=False, layers_cover_min=0.5, score=False, score_iou=0.5,
                 score_truth=None, identity=False, identity_iou=0.3, identity_tracks=None, identity_max_age=10, identity_reid_dist=4.0,
                 identity_reid_what=float("inf"), identity_appearance=True, score_ids="row"):
        if core.cfg.sample_from_prior:
            raise ValueError("SqairStream: generation modes (sample_from_prior) do not carry a state across calls")
        if resample not in (None, "systematic"):
            raise ValueError("SqairStream: resample must be None or 'systematic'")
        ess_frac = float(ess_frac)
        if resample is not None and not 0.0 <= ess_frac <= 1.0:   # (NaN fails too)
            raise ValueError("SqairStream: ess_frac must lie in [0, 1]")
        estimate_iou = float(estimate_iou)
        if estimate and not 0.0 < estimate_iou <= 1.0:   # (NaN fails too)
            raise ValueError("SqairStream: estimate_iou must lie in (0, 1]")
        if estimate_canvas and not estimate:
            raise ValueError("SqairStream: estimate_canvas is for a stream with estimate=True")
        if estimate_layers and not estimate:
            raise ValueError("SqairStream: estimate_layers is for a stream with estimate=True")
        layers_cover_min = float(layers_cover_min)
        if estimate_layers and not 0.0 < layers_cover_min <= 1.0:   # (NaN fails too)
            raise ValueError("SqairStream: layers_cover_min must lie in (0, 1]")
        if score and not estimate:
            raise ValueError("SqairStream: score is for a stream with estimate=True")
        score_iou = float(score_iou)
        if score and not 0.0 < score_iou <= 1.0:   # (NaN fails too)
            raise ValueError("SqairStream: score_iou must lie in (0, 1]")
        if score and score_truth is not None and (isinstance(score_truth, bool) or not isinstance(score_truth, (int, np.integer)) or
                                                  not 1 <= score_truth <= _capi.SCORE_MAX_TRUTH):
            raise ValueError("SqairStream: score_truth must be an integer in [1, {}]".format(_capi.SCORE_MAX_TRUTH))
        if identity and not estimate:
            raise ValueError("SqairStream: identity is for a stream with estimate=True")
        identity_iou, identity_reid_dist, identity_reid_what = float(identity_iou), float(identity_reid_dist), float(identity_reid_what)
        if identity and not 0.0 < identity_iou <= 1.0:   # (NaN fails too)
            raise ValueError("SqairStream: identity_iou must lie in (0, 1]")
        if identity and identity_tracks is not None and (isinstance(identity_tracks, bool) or not isinstance(identity_tracks, (int, np.integer)) or
                                                         not 1 <= identity_tracks <= _capi.IDENT_MAX_TRACKS):
            raise ValueError("SqairStream: identity_tracks must be an integer in [n_steps_per_image, {}]".format(_capi.IDENT_MAX_TRACKS))
        if identity and (isinstance(identity_max_age, bool) or not isinstance(identity_max_age, (int, np.integer)) or identity_max_age < 0):
            raise ValueError("SqairStream: identity_max_age must be an integer >= 0")
        if identity and not identity_reid_dist >= 0.0:   # (NaN fails too)
            raise ValueError("SqairStream: identity_reid_dist must be >= 0")
        if identity and not identity_reid_what > 0.0:   # (NaN fails too)
            raise ValueError("SqairStream: identity_reid_what must lie in (0, +inf]")
        if score_ids not in ("row", "lane"):
            raise ValueError("SqairStream: score_ids must be 'row' or 'lane'")
        if score_ids == "lane" and not (score and identity):
            raise ValueError("SqairStream: score_ids='lane' is for a stream with score=True and identity=True")
        self.smc = resample is not None
        self.ess_frac = ess_frac
        self.core = core
        self.B, self.K = int(B), core.K
        self.R = self.B * self.K
        self.T = int(frames_per_step)
        if self.B < 1 or self.T < 1:
            raise ValueError("SqairStream: B and frames_per_step must be >= 1")
        self.identified = bool(identity)
        self.M = (min(_capi.IDENT_MAX_TRACKS, 2 * core.N) if identity_tracks is None else int(identity_tracks)) if self.identified else 0   # track entries per lane
        if self.identified and not core.N <= self.M:   # (the last check that needs the core's N: still before the handle is touched)
            raise ValueError("SqairStream: identity_tracks must be an integer in [n_steps_per_image, {}]".format(_capi.IDENT_MAX_TRACKS))
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
        self._traj = {}             # trajectory scores by kind ("forecast", "tracks"): accumulators and outputs of the LAST (F, G, truth_iou)
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
        self.estimate = bool(estimate)
        self.scored = bool(score)
        self.G = (core.N if score_truth is None else int(score_truth)) if self.scored else 0   # truth slots per lane
        if self.estimate:   # after SMC: the estimate's log_w must be the resampler's accumulator
            self._est = self._estimate_buffers(bool(estimate_canvas), bool(estimate_layers), self.G, self.identified)
            est = _capi.SqairLaneEstimate(iou_min=estimate_iou, log_w=cs.log_weight_sum.data_ptr(),
                                          **{n: t.data_ptr() for n, t in self._est.items() if n in _capi.ESTIMATE_FIELDS})
            torch.cuda.current_stream(core.device).synchronize()
            core.check(core.lib.sqair_set_estimate(core.handle, C.byref(est), self.T, self.B), "sqair_set_estimate")
            if estimate_layers:
                lay = _capi.SqairLaneLayers(cover_min=layers_cover_min, **{n: self._est[n].data_ptr() for n in _capi.LAYERS_FIELDS})
                core.check(core.lib.sqair_set_layers(core.handle, C.byref(lay), self.T, self.B), "sqair_set_layers")
            if self.scored:   # the truth of a step, the accumulators and the identity memory: the stream's own device buffers
                z = lambda shp, dt: torch.zeros(shp, dtype=dt, device=core.device)
                self._score = dict(truth_box=z((self.T, self.B, self.G, 4), torch.float32), truth_present=z((self.T, self.B, self.G), torch.int32),
                                   truth_valid=z((self.T, self.B), torch.int32), counts=z((self.B, len(_capi.SCORE_COUNTS)), torch.int64),
                                   iou_sum=z((self.B,), torch.float64), last_id=z((self.B, self.G), torch.int32) - 1)
                self._score_valid_is_zero = True
                sc = _capi.SqairLaneScore(iou_min=score_iou, G=self.G, **{n: t.data_ptr() for n, t in self._score.items()},
                                          **{n: self._est[n].data_ptr() for n in _capi.SCORE_FIELDS})
                torch.cuda.current_stream(core.device).synchronize()
                core.check(core.lib.sqair_set_score(core.handle, C.byref(sc), self.T, self.B), "sqair_set_score")
            if self.identified:   # the track table of every lane and the counters: the stream's own device buffers
                shapes = _capi.identity_memory_shapes(self.B, self.M, core.nw)
                if not identity_appearance:
                    del shapes["trk_what"]
                floats = ("trk_box", "trk_what")
                self._ident = {n: torch.zeros(shp, dtype=torch.float32 if n in floats else torch.int64 if n == "counts" else torch.int32,
                                              device=core.device) for n, shp in shapes.items()}
                self._ident["trk_id"].fill_(-1)
                idt = _capi.SqairLaneIdentity(iou_min=identity_iou, reid_dist=identity_reid_dist, reid_what=identity_reid_what, M=self.M,
                                              max_age=int(identity_max_age), **{n: t.data_ptr() for n, t in self._ident.items()},
                                              **{n: self._est[_capi.IDENT_LANE_NAMES[n]].data_ptr() for n in _capi.IDENT_FIELDS})
                torch.cuda.current_stream(core.device).synchronize()
                core.check(core.lib.sqair_set_identity(core.handle, C.byref(idt), self.T, self.B), "sqair_set_identity")
                if score_ids == "lane":
                    core.check(core.lib.sqair_set_score_ids(core.handle, 1), "sqair_set_score_ids")
        if history is not None:
            ring, nb, bits = cs.set_history(history, history_fields, self.T)
            torch.cuda.current_stream(core.device).synchronize()   # (the ring's zeros are in place before a pass pushes into it)
            core.check(core.lib.sqair_set_history(core.handle, ring.data_ptr(), nb, cs.history, bits), "sqair_set_history")
        core._graph_ready = False   # (the handle's graph is now this stream's)

    # the carried state's, read-only (_src, _armed, _src_is_identity: what the tests and tools look at)
    state, log_weight_sum, log_z, log_evidence, ess, u, resampled, _src, _armed, _src_is_identity, history, history_fields = (
        carried(n) for n in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src", "_armed",
                             "_src_is_identity", "history", "history_fields"))

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

    def _estimate_buffers(self, canvas, layers=False, score_truth=0, identity=False):
        """The device buffers k_lane_estimate -- and, with ``layers``, k_lane_layers, with ``score_truth`` = G > 0, k_lane_score's
        per-frame outputs, with ``identity`` k_lane_identity's -- writes (include/sqair_hip.h: SqairLaneEstimate, SqairLaneLayers,
        SqairLaneScore, SqairLaneIdentity), by field: views of ONE allocation (``_est_flat``), so that a step copies them out with one
        launch instead of one per field."""
        core = self.core
        shapes = _capi.estimate_shapes(self.T, self.B, self.K, core.N, core.nw, (core.H, core.W) if canvas else None)
        if layers:
            shapes.update(_capi.layers_shapes(self.T, self.B, self.K, core.N, (core.H, core.W)))
        if score_truth:
            shapes.update(_capi.score_shapes(self.T, self.B, score_truth))
        ints = _capi.ESTIMATE_INT_FIELDS + (_capi.LAYERS_INT_FIELDS if layers else ()) + (_capi.SCORE_INT_FIELDS if score_truth else ())
        if identity:
            shapes.update(_capi.identity_shapes(self.T, self.B, core.N))
            ints = ints + tuple(_capi.IDENT_LANE_NAMES[n] for n in _capi.IDENT_FIELDS)
        self._est_flat, self._est_views = _field_views(shapes, ints, core.device)
        return self._est_views(self._est_flat)

    # ---- source map -------------------------------------------------------------------------------------------------------
    def reset(self, lanes):
        """Lanes (sequences, in [0, B)) whose next step starts a new clip: their K particle rows start fresh, counter 0.  A scored
        stream also forgets those lanes' identities (``last_id``: a new clip has new ones); their counters stay.  A stream with
        ``identity=True`` frees those lanes' track entries (``trk_id`` = -1) and keeps their ``next_id``: an id is never reused within
        a lane."""
        self.carried.reset(lanes)
        if self.scored or self.identified:
            lanes = sorted(set(self.carried.check_lanes(lanes)))
            if lanes:
                with self.carried._on_core_stream():
                    for j in lanes:
                        if self.scored:
                            self._score["last_id"][j].fill_(-1)
                        if self.identified:
                            self._ident["trk_id"][j].fill_(-1)

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

    def _check_truth(self, truth):
        """``truth`` of a step as (box float32 [T', B, G, 4], present int32 [T', B, G], valid int32 [T', B]) (None: no truth)."""
        if truth is None:
            return None
        fn = "SqairStream.step: "
        if not self.scored:
            raise ValueError(fn + "truth is for a stream with score=True")
        if not isinstance(truth, dict) or "box" not in truth or "present" not in truth or set(truth) - {"box", "present", "valid"}:
            raise ValueError(fn + "truth must be a dict with box, present and optionally valid")
        T, B, G = self.T, self.B, self.G
        box = torch.as_tensor(truth["box"]).to(torch.float32)
        present = torch.as_tensor(truth["present"])
        valid = truth.get("valid")
        valid = torch.ones((T, B), dtype=torch.int32) if valid is None else torch.as_tensor(valid)
        if T == 1 and box.dim() == 3:
            box, present, valid = box[None], present[None], (valid[None] if valid.dim() == 1 else valid)
        for name, t, shp in (("box", box, (T, B, G, 4)), ("present", present, (T, B, G)), ("valid", valid, (T, B))):
            if tuple(t.shape) != shp:
                raise ValueError(fn + "truth[{!r}] of shape {} given, {} expected".format(name, tuple(t.shape), list(shp)))
        as_mask = lambda m: m if m.dtype == torch.int32 else (m != 0).to(torch.int32)   # (the kernel tests != 0: int32 goes as it is)
        return box, as_mask(present), as_mask(valid)

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
        with [B, ...] accepted when T' = 1; the step's lane answer is scored against it.  Default: nothing is scored."""
        observed = self._check_observed(observed)   # (before the core is touched)
        truth = self._check_truth(truth)
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
                if self.scored:   # (as the mask: the kernel reads the stream's own buffers, so one graph serves every step)
                    if truth is not None:
                        for n, t in zip(("truth_box", "truth_present", "truth_valid"), truth):
                            self._score[n].copy_(t, non_blocking=True)
                    elif not self._score_valid_is_zero:
                        self._score["truth_valid"].zero_()
                    self._score_valid_is_zero = truth is None
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
                    out["lane"] = self._est_views(self._est_flat.clone())
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
        if not self.scored:
            raise ValueError("SqairStream.score: the stream keeps no score (SqairStream(..., estimate=True, score=True))")
        core = self.core
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                counts, iou_sum = self._score["counts"].clone(), self._score["iou_sum"].clone()
                if reset:
                    self._score["counts"].zero_()
                    self._score["iou_sum"].zero_()
            core._join_out()
            counts, iou_sum = counts.cpu(), iou_sum.cpu()
        res = {n: counts[:, i].clone() for i, n in enumerate(_capi.SCORE_COUNTS)}
        res["iou_sum"] = iou_sum
        tot = {n: int(v.sum()) for n, v in res.items() if n != "iou_sum"}
        div = lambda a, b: float(a) / b if b else float("nan")
        res["mota"] = 1.0 - div(tot["fn"] + tot["fp"] + tot["idsw"], tot["truth"])
        res["motp"] = div(float(iou_sum.sum()), tot["tp"])
        res["count_accuracy"] = div(tot["count_hit"], tot["frames"])
        return res

    # ---- lane identities --------------------------------------------------------------------------------------------------
    def identities(self):
        """The identities so far (include/sqair_hip.h: sqair_set_identity): per lane the int64 counters ``frames``, ``frames_invalid``,
        ``objects``, ``kept``, ``bridged``, ``reidentified``, ``born``, ``ended`` [B] and ``next_id`` [B]; pooled over the lanes
        ``bridged_rate`` = bridged / objects and ``reidentified_rate`` = reidentified / objects (NaN without objects); and the track
        table ``trk_id``, ``trk_age``, ``trk_len`` [B, M] and ``trk_box`` [B, M, 4] (host tensors): the entries with ``trk_id`` >= 0 and
        ``trk_age`` > 0 are the tracks remembered but currently unseen."""
        if not self.identified:
            raise ValueError("SqairStream.identities: the stream keeps no identities (SqairStream(..., estimate=True, identity=True))")
        core = self.core
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                got = {n: self._ident[n].clone() for n in ("counts", "next_id", "trk_id", "trk_age", "trk_len", "trk_box")}
            core._join_out()
            got = {n: v.cpu() for n, v in got.items()}
        counts = got.pop("counts")
        res = {n: counts[:, i].clone() for i, n in enumerate(_capi.IDENT_COUNTS)}
        tot = {n: int(v.sum()) for n, v in res.items()}
        div = lambda a, b: float(a) / b if b else float("nan")
        res.update(got)
        res["bridged_rate"] = div(tot["bridged"], tot["objects"])
        res["reidentified_rate"] = div(tot["reidentified"], tot["objects"])
        return res

    # ---- trajectory scoring ------------------------------------------------------------------------------------------------
    def _check_traj_truth(self, fn, truth, lane, F, default_anchor, link_ids, truth_iou):
        """``truth`` of ``forecast`` / ``tracks`` as {name: tensor} in the C ABI's names and dtypes plus ``G`` and ``iou_min`` (None: no
        truth); everything is checked here, before the core is touched."""
        if truth is None:
            if link_ids:
                raise ValueError(fn + "link_ids is for a call with truth")
            return None
        if not lane:
            raise ValueError(fn + "truth is for a call with lane=True: the lane table is what is scored")
        names = {"box", "present", "valid", "anchor_box", "anchor_present", "anchor_valid"}
        if not isinstance(truth, dict) or "box" not in truth or "present" not in truth or set(truth) - names:
            raise ValueError(fn + "truth must be a dict with box, present and optionally valid, anchor_box, anchor_present, anchor_valid")
        truth_iou = float(truth_iou)
        if not 0.0 < truth_iou <= 1.0:   # (NaN fails too)
            raise ValueError(fn + "truth_iou must lie in (0, 1]")
        B = self.B
        box = torch.as_tensor(truth["box"]).to(torch.float32)
        present = torch.as_tensor(truth["present"])
        if box.dim() != 4 or not 1 <= box.shape[2] <= _capi.SCORE_MAX_TRUTH:
            raise ValueError(fn + "truth['box'] of shape {} given, [{}, {}, G, 4] with G in [1, {}] expected".format(
                tuple(box.shape), F, B, _capi.SCORE_MAX_TRUTH))
        G = int(box.shape[2])
        def shaped(items):
            for name, t, shp in items:
                if tuple(t.shape) != shp:
                    raise ValueError(fn + "truth[{!r}] of shape {} given, {} expected".format(name, tuple(t.shape), list(shp)))
        given = truth.get("valid") is not None
        valid = torch.as_tensor(truth["valid"]) if given else torch.ones((F, B), dtype=torch.int32)
        shaped((("box", box, (F, B, G, 4)), ("present", present, (F, B, G)), ("valid", valid, (F, B))))
        if (truth.get("anchor_box") is None) != (truth.get("anchor_present") is None):
            raise ValueError(fn + "truth['anchor_box'] and truth['anchor_present'] come together")
        a_valid = truth.get("anchor_valid")
        if truth.get("anchor_box") is None:
            if not default_anchor:
                raise ValueError(fn + "a forecast's truth needs anchor_box and anchor_present: the truth at the last stepped frame, "
                                      "which is none of the forecast's frames")
            a_box, a_present = box[-1], present[-1]   # (a trace's newest frame is the last stepped one)
            if a_valid is None and given:
                a_valid = valid[-1]
        else:
            a_box, a_present = torch.as_tensor(truth["anchor_box"]).to(torch.float32), torch.as_tensor(truth["anchor_present"])
        a_valid = torch.ones((B,), dtype=torch.int32) if a_valid is None else torch.as_tensor(a_valid)
        shaped((("anchor_box", a_box, (B, G, 4)), ("anchor_present", a_present, (B, G)), ("anchor_valid", a_valid, (B,))))
        if link_ids and not (self.scored and G == self.G):
            raise ValueError(fn + "link_ids is for a stream with score=True and the same G: it keeps a truth with the identity the "
                                  "stream's score last matched it with")
        as_mask = lambda m: m if m.dtype == torch.int32 else (m != 0).to(torch.int32)
        return dict(G=G, iou_min=truth_iou, truth_box=box, truth_present=as_mask(present), truth_valid=as_mask(valid), anchor_box=a_box,
                    anchor_present=as_mask(a_present), anchor_valid=as_mask(a_valid))

    def _traj_score(self, kind, table, F, truth, link_ids):
        """Scores the lane table a forecast or a trace has just written (``table``: its device buffers by field) against ``truth``
        (of _check_traj_truth) with one launch on the core's stream (include/sqair_hip.h: sqair_lane_traj_score); returns the
        per-call outputs, copies.  The accumulators of ``kind`` are kept for the last (F, G, truth_iou) scored."""
        core = self.core
        G, key = truth["G"], (F, truth["G"], truth["iou_min"])
        ts = self._traj.get(kind)
        if ts is None or ts["key"] != key:   # (another F, G or threshold: the old sums would not mean the same)
            z = lambda shp, dt: torch.zeros(shp, dtype=dt, device=core.device)
            ts = self._traj[kind] = dict(key=key, counts=z((F, self.B, len(_capi.TRAJ_COUNTS)), torch.int64),
                                         sums=z((F, self.B, len(_capi.TRAJ_SUMS)), torch.float64),
                                         lane_counts=z((self.B, len(_capi.TRAJ_LANE_COUNTS)), torch.int64))
            ts["flat"], ts["views"] = _field_views(_capi.traj_shapes(F, self.B, G), _capi.TRAJ_INT_FIELDS, core.device)
            ts["out"] = ts["views"](ts["flat"])
        dev = {n: truth[n].to(core.device, non_blocking=True).contiguous() for n in _capi.TRAJ_TRUTH_FIELDS if n != "keep_id"}
        c_tab = _capi.SqairLaneTraj(**{n: table[n].data_ptr() for n in _capi.TRAJ_TABLE_FIELDS if n in table})
        c_truth = _capi.SqairTrajTruth(G=G, keep_id=self._score["last_id"].data_ptr() if link_ids else None,
                                       **{n: t.data_ptr() for n, t in dev.items()})
        c_score = _capi.SqairTrajScore(iou_min=truth["iou_min"], **{n: ts[n].data_ptr() for n in _capi.TRAJ_ACCUMULATORS},
                                       **{n: t.data_ptr() for n, t in ts["out"].items()})
        core.check(core.lib.sqair_lane_traj_score(core.handle, C.byref(c_tab), C.byref(c_truth), C.byref(c_score), F, self.B,
                                                  core._stream()), "sqair_lane_traj_score")
        return ts["views"](ts["flat"].clone())

    def trajectory_score(self, kind, reset=False):
        """The trajectory score so far of ``kind`` = "forecast" or "tracks" (include/sqair_hip.h: sqair_lane_traj_score): what the
        calls with ``truth`` have accumulated.  Per (frame or horizon f, lane) the int64 counters ``frames``, ``pairs``, ``hits``,
        ``lost``, ``gone``, ``count_hit``, ``count_abs_err`` [F, B] and the fp64 ``iou_sum``, ``centre_err_sum``, ``brier_sum`` [F, B]; per
        lane ``calls``, ``calls_invalid``, ``anchor_truth``, ``linked`` [B] (host tensors).  Pooled over the lanes, per f, NaN where the
        denominator is 0: ``ade`` = centre_err_sum / pairs (``fde`` = its last entry), ``mean_iou`` = iou_sum / pairs, ``hit_rate`` =
        hits / (pairs + lost), ``brier`` = brier_sum / (pairs + lost + gone), ``count_accuracy`` = count_hit / frames [F] (float64), and
        ``link_rate`` = linked / anchor_truth.  The accumulators belong to (kind, F, G, truth_iou): a call with truth of another F, G
        or threshold starts fresh ones and drops the old.  ``reset``: they start again from zero afterwards."""
        if kind not in ("forecast", "tracks"):
            raise ValueError("SqairStream.trajectory_score: kind must be 'forecast' or 'tracks'")
        ts = self._traj.get(kind)
        if ts is None:
            raise ValueError("SqairStream.trajectory_score: no {} call has been scored yet ({}(..., lane=True, truth=...))".format(kind, kind))
        core = self.core
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                acc = {n: ts[n].clone() for n in _capi.TRAJ_ACCUMULATORS}
                if reset:
                    for n in _capi.TRAJ_ACCUMULATORS:
                        ts[n].zero_()
            core._join_out()
            acc = {n: t.cpu() for n, t in acc.items()}
        res = {n: acc["counts"][..., i].clone() for i, n in enumerate(_capi.TRAJ_COUNTS)}
        res.update({n: acc["sums"][..., i].clone() for i, n in enumerate(_capi.TRAJ_SUMS)})
        res.update({n: acc["lane_counts"][:, i].clone() for i, n in enumerate(_capi.TRAJ_LANE_COUNTS)})
        tot = {n: res[n].sum(1).to(torch.float64) for n in _capi.TRAJ_COUNTS + _capi.TRAJ_SUMS}
        div = lambda a, b: torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), torch.full_like(b, float("nan")))
        res["ade"] = div(tot["centre_err_sum"], tot["pairs"])
        res["fde"] = float(res["ade"][-1])
        res["mean_iou"] = div(tot["iou_sum"], tot["pairs"])
        res["hit_rate"] = div(tot["hits"], tot["pairs"] + tot["lost"])
        res["brier"] = div(tot["brier_sum"], tot["pairs"] + tot["lost"] + tot["gone"])
        res["count_accuracy"] = div(tot["count_hit"], tot["frames"])
        linked, anchors = int(res["linked"].sum()), int(res["anchor_truth"].sum())
        res["link_rate"] = float(linked) / anchors if anchors else float("nan")
        return res

    # ---- forecasting ------------------------------------------------------------------------------------------------------
    def forecast(self, F, noise=None, seed=None, outputs=FORECAST_OUTPUTS, summaries=True, samples=1, lane=False, lane_iou=0.5,
                 truth=None, link_ids=False, truth_iou=0.5):
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
        with ``score=True`` and the same G) keeps each truth with the identity the stream's score last matched it with.  Without
        ``truth`` nothing is launched, and with it every other output is unchanged bit for bit."""
        F, S, lane, lane_iou = int(F), int(samples), bool(lane), float(lane_iou)
        if F < 1:
            raise ValueError("SqairStream.forecast: F must be >= 1")
        if S < 1 or self.K * S > _capi.FORECAST_FAN_MAX:
            raise ValueError("SqairStream.forecast: samples must be >= 1 with K * samples <= {}".format(_capi.FORECAST_FAN_MAX))
        if lane and not 0.0 < lane_iou <= 1.0:   # (NaN fails too)
            raise ValueError("SqairStream.forecast: lane_iou must lie in (0, 1]")
        outputs = tuple(outputs)
        bad = [n for n in outputs if n not in FORECAST_OUTPUTS]
        if bad:
            raise ValueError("SqairStream.forecast: unknown outputs {} (choose from {})".format(bad, FORECAST_OUTPUTS))
        truth = self._check_traj_truth("SqairStream.forecast: ", truth, lane, F, False, link_ids, truth_iou)
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
                score = None if truth is None else self._traj_score("forecast", fc["lane"], F, truth, link_ids)
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
                  out={n: z(shapes[n]) for n in outputs})
        if lane:   # the fields of SqairForecastLane as views of ONE allocation
            fc["lane_flat"], fc["lane_views"] = _field_views(_capi.forecast_lane_shapes(F, B, self.K, N), _capi.FORECAST_LANE_INT_FIELDS,
                                                             core.device)
            fc["lane"] = fc["lane_views"](fc["lane_flat"])
        return fc

    # ---- track history ----------------------------------------------------------------------------------------------------
    def tracks(self, lag=None, start="next", max_tracks=None, table=True, lane=False, lane_iou=0.5, truth=None, link_ids=False,
               truth_iou=0.5):
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
        if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 1 <= lag <= cs.history:
            raise ValueError("SqairStream.tracks: lag must be an integer in [1, history = {}]".format(cs.history))
        if start not in ("next", "last"):
            raise ValueError("SqairStream.tracks: start must be 'next' or 'last'")
        M = 2 * core.N if max_tracks is None else max_tracks
        if table and (isinstance(M, bool) or not isinstance(M, (int, np.integer)) or not 1 <= M <= 1024):
            raise ValueError("SqairStream.tracks: max_tracks must be an integer in [1, 1024]")
        lane, lane_iou = bool(lane), float(lane_iou)
        if lane and start != "next":
            raise ValueError("SqairStream.tracks: lane=True requires start='next': the lane answer is weighed by the weights of the rows "
                             "the next step starts from, as forecast()'s is")
        if lane and not 0.0 < lane_iou <= 1.0:   # (NaN fails too)
            raise ValueError("SqairStream.tracks: lane_iou must lie in (0, 1]")
        lag, M = int(lag), int(M)
        truth = self._check_traj_truth("SqairStream.tracks: ", truth, lane, lag * self.T, True, link_ids, truth_iou)
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
                score = None if truth is None else self._traj_score("tracks", tr["lane"], lag * self.T, truth, link_ids)
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
        i32 = torch.int32
        shapes = dict(where=((F, R, N, 4), None), presence=((F, R, N), None), obj_id=((F, R, N), None), valid=((F, R), i32),
                      frame_index=((F, R), i32), ancestor_row=((lag, R), i32), unique_ancestors=((lag, B), i32))
        if "what" in self.history_fields:
            shapes["what"] = ((F, R, N, core.nw), None)
        if "log_weights_per_timestep" in self.history_fields:
            shapes["log_w"] = ((F, R), None)
        if table:
            shapes.update(track_id=((R, M), i32), n_tracks=((R,), i32), track_present=((F, R, M), None),
                          track_where=((F, R, M, 4), None))
        z = lambda shp, dt=None: torch.zeros(shp, dtype=dt or torch.float32, device=core.device)
        tr = dict(src=z(R, i32), log_w=z(R), out={n: z(*sd) for n, sd in shapes.items()})
        if lane:   # the fields of SqairTraceLane as views of ONE allocation, and the scratch between the two lane launches
            tr["lane_flat"], tr["lane_views"] = _field_views(_capi.track_lane_shapes(F, B, self.K, N), _capi.TRACK_LANE_INT_FIELDS,
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
            core._graph_ready = False
