"""The lane answers of a stream, host side: what ``SqairStream`` (sqair_amd/stream.py) says per lane instead of per particle row.
``LaneAnswers`` is the resident stack a step fills -- the estimate and its followers, each one more kernel of the pass
(include/sqair_hip.h states the semantics; sqair_amd/csrc/sqair_lane_api.hip registers and launches them as one block) --,
``TrajScores`` the per-call trajectory scores of ``forecast`` and ``tracks``.  The stream owns one of each and keeps its public surface.

``estimate=True``: a step also returns ``out["lane"]``, one answer per lane and frame from the K particles, formed before the
resampler zeroes the weights (sqair_set_estimate): the normalised ``weights`` [T', B, K] and ``ess`` [T', B] of the step's own rows,
``best_row``, the count posterior ``count_prob`` [T', B, N + 1] with ``expected_count`` and ``map_count``, the best row's objects
(``presence``, ``obj_id``, ``where``, ``what``) with their ``box`` [T', B, N, 4] = (y, x, h, w) in pixels, and per object the
``support`` -- the weight of the particles that hold a box of IoU >= ``estimate_iou`` with it -- and their weighted mean box
``box_mean``; with ``estimate_canvas`` the posterior mean reconstruction ``mean_canvas`` [T', B, H, W].

``estimate_layers=True``: ``out["lane"]`` also says which pixels each object of the lane occupies (sqair_set_layers): ``match``
[T', B, K, N] -- the slot of particle k associated with object j, -1 where it does not agree -- and, over the particles that agree,
the weighted mean of what the decoder drew for the object: its appearance ``layer`` and its coverage ``cover`` [T', B, N, H, W];
``owner`` [T', B, H, W] is the object of largest coverage at a pixel, -1 (background) below ``layers_cover_min``.

``score=True``: the lane answer is scored against ground-truth boxes inside the pass (sqair_set_score): a step takes
``truth=dict(box=[T', B, G, 4], present=[T', B, G], valid=[T', B] or None)`` -- (y, x, h, w) in pixels as ``make_sequences``'s
``coords``, G = ``score_truth`` slots per lane, an object keeping its slot for its life -- copied into stream-owned device buffers
the way ``observed`` is; a step without ``truth`` scores nothing.  Present truths and present lane objects of IoU >= ``score_iou``
are matched one to one (an object's last identity first, then greedily by IoU -- or, with ``score_match="optimal"``, as many pairs as
possible and among those the largest total IoU, CLEAR-MOT's own rule: sqair_set_lane_match) and the CLEAR-MOT events counted on the device:
``out["lane"]`` gains ``truth_match``, ``match_iou`` [T', B, G] and ``tp``, ``fn``, ``fp``, ``idsw`` [T', B] (-1 where nothing was
scored), and ``score()`` reads the accumulators.  ``reset(lanes)`` also forgets those lanes' identities (a new clip has new ones)
and keeps their counters.

``identity=True``: every object of the lane answer carries a track id that stays on it for as long as the tracker can tell it is the
same object (sqair_set_identity), formed after the layers and before the score.  ``obj_id`` is the best row's per-row counter and
changes when the best row switches; ``lane_id`` does not: a table of ``identity_tracks`` (default min(16, 2 N)) tracks per lane is
kept on the device, and each frame's objects are linked to it by position (IoU >= ``identity_iou``, the same obj_id first), then --
``identity_reid_dist`` > 0 -- an object that was dropped for up to ``identity_max_age`` frames is re-identified when its centre lies
within ``identity_reid_dist`` pixels per frame unseen and, with ``identity_appearance``, its ``what`` within ``identity_reid_what``
of the track's (the nearest appearance wins), else it is born under a fresh id.  ``out["lane"]`` gains ``lane_id``, ``id_how``
(0 born, 1 kept, 2 bridged -- the obj_id changed under it --, 3 re-identified) and ``track_len`` [T', B, N] int32, -1 where the slot
is absent; ``identities()`` reads the counters and the table.  ``reset(lanes)`` frees those lanes' tracks; ids are never reused
within a lane.  ``score_ids="lane"`` (with ``score=True``) makes the score count its identity switches on ``lane_id`` instead of
``obj_id``.  ``identity_match="optimal"`` makes the position link keep + optimal where it is keep + greedy (sqair_set_lane_match);
re-identification, births and ageing are the same either way.

``motion=True`` (with ``identity=True``): every track also carries a constant-velocity Kalman filter of its box centre, inside the
identity's kernel (sqair_set_motion: the same node, no launch more).  The position link then compares a slot with the track's
PREDICTED box, and re-identification gates on the normalised innovation -- d2 <= ``motion_gate``^2 sigmas -- where it searched a disc
of ``identity_reid_dist`` pixels per frame unseen (``identity_reid_dist`` > 0 stays its on/off switch): a fast object keeps its id,
and an object that moved while unseen is found where it went.  ``motion_q`` is the white-acceleration variance, ``motion_r`` the
measurement variance in px^2, ``motion_v0`` the velocity variance of a newborn track.  ``out["lane"]`` gains ``velocity``
[T', B, N, 2] = (v_y, v_x) in pixels per frame, 0 for an absent slot and a newborn, and with ``motion_nis=True`` also ``nis`` [T', B, N],
the d2 of the pair each slot was linked through.  ``identities()`` gains ``trk_centre``, ``trk_vel``, ``trk_sigma`` [B, M, 2]
(= sqrt(Ppp)) and ``trk_pred_box`` [B, M, 4], the coasted box of every live track: for ``trk_age`` > 0 that is where the filter
thinks the unseen object is.

``tracklog=L`` (with ``identity=True``): the stream keeps, per lane and on the device, the last L frames of ``lane_id``,
``track_len`` and ``box`` in a ring, written by one more kernel of the pass directly behind the identity's (sqair_set_tracklog), and
``track_log(lag)`` turns the last ``lag`` of them into one trajectory per ``lane_id`` with one launch (sqair_lane_tracklog_smooth):
up to ``tracklog_tracks`` track columns, the newest ids, each filtered forward by the motion's constant-velocity model and smoothed
backward (Rauch-Tung-Striebel), so that a frame in which the object was not seen holds the model's interpolation instead of a
hole and a track that ended is still there.  It does not need ``motion=True``.  ``reset(lanes)`` empties those lanes' logs.
``mot_rows(log, lane)`` lists a lane's smoothed boxes as MOTChallenge rows.

``tracklog_truth=G`` (with ``tracklog=L``): the stream also keeps the truth of the last L stepped frames in a ring on the device --
a step's ``truth`` (accepted then without ``score=True``) goes to position (frames stepped + t) mod L by small copies beside the
score's, outside the captured graph; a step without truth leaves its positions invalid -- and ``track_log(lag, score=True)`` scores
the log against it with one more launch behind the solve (sqair_lane_tracklog_score): four views of the one table -- ``filtered``
and ``smooth``, each as reported and with the gaps filled -- each with the CLEAR-MOT events, the identity measures over the window,
the centre error of every matched pair and its normalised square (``nees``, 2 for an honest sigma), and the same figures over the
filled gaps alone: whether gap filling turned misses into hits or into false positives, whether smoothing moved the boxes towards
the truth, whether sigma is honest.  Window frame f of every lane is stream frame (frames stepped - lag + f), whatever the lane's
own ``count`` says after a ``reset(lanes)``, so one gather of the ring serves all lanes; ``reset(lanes)`` leaves the ring alone.

``track_log_fit()`` (a stream with ``tracklog=L``; no truth needed) picks the filter's ``q`` and ``r`` from the log itself: one more
launch behind the solve (sqair_lane_tracklog_fit) walks every track of the window under every (q, r) of a grid and sums the filter's
normalised innovations and log-variances; ``track_log_fit(got, q_grid, r_grid)`` here forms the negative log-likelihood of every
node, its minimum -- the maximum-likelihood fit on the grid -- and ``mean_nis``, 1 for an honest filter.  ``set_motion(q, r)`` applies
a fit: the defaults of ``track_log()`` and ``track_log_fit()`` follow, and on a stream with ``motion=True`` the following steps' filter.

``track_log(lag, stitch=True)`` joins the fragments one object left in the log under several ids: one more launch behind the solve
(sqair_lane_tracklog_stitch) links a column that ended to a column born later when the old one's coasted state and the new one's
smoothed state at birth agree within ``stitch_gate`` sigmas, one to one, and solves the joined columns again; the result gains
``stitched`` -- the same keys for the stitched table, ``links``, and with ``score=True`` its own ``score``.

``score_idf=True`` (with ``score=True``): the score's idsw counts the moments an identity changes, not for how long the wrong id then
stays.  The stream then also keeps, per lane and on the device, how many frames of the open clip every truth overlapped (IoU >=
``score_iou``) every predicted id -- the id words the score reads: ``obj_id``, or ``lane_id`` with ``score_ids="lane"`` --, up to
``score_idf_ids`` ids per clip, one more kernel of the pass after the score's (sqair_set_idf); ``idf_score()`` solves the maximum-weight
one-to-one assignment of truths to ids on the device (sqair_lane_idf_solve) and returns IDF1, IDP, IDR, mostly tracked / partly
tracked / mostly lost and the fragmentations.  ``reset(lanes)`` closes those lanes' clips -- their figures go into the totals and
their tables are freed -- before it forgets their identities: a new clip has new truth identities.

``score_hota=True`` (with ``score=True``): CLEAR-MOT is dominated by detection, IDF1 by association; HOTA separates detection,
association and localisation and combines them.  It needs two passes over a clip, so the stream keeps a per-lane clip log on the
device -- per scored frame the IoU of every (truth, keyed lane object) pair in units of 2^-20, the objects' id columns (up to
``score_hota_ids`` per clip, the IDF's column rule) and the truths present, up to ``score_hota_frames`` frames per clip -- with one
more kernel of the pass after the score's and the IDF's (sqair_set_hota); ``hota_score()`` makes both passes on the device
(sqair_lane_hota_solve) and returns HOTA, DetA, AssA, LocA and their parts.  ``reset(lanes)`` closes those lanes' clips as it does
the IDF's.

``forecast(..., lane=True, truth=...)`` and ``tracks(..., lane=True, truth=...)`` score the two answers that reach over time -- the
lane forecast and the lane tracks -- against the truth's trajectories with one more launch after the call's own
(sqair_lane_traj_score): truth and lane objects are linked once, at the last stepped frame, and every horizon or traced frame then
(``link_match="optimal"``: by keep + optimal, sqair_set_lane_match) gives displacement error, IoU, the Brier term of ``alive / support`` as a survival probability and the count's hit, accumulated on
the device per (frame, lane); ``trajectory_score(kind)`` reads the sums and pools them into curves over the horizon without a lane
table ever visiting the host."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from sqair_amd import _capi


MATCH_MODES = ("greedy", "optimal")   # the values of sqair_set_lane_match, by index (include/sqair_hip.h)


def lane_answer(name, of="lane"):
    """A read-only attribute of a stream class that is attribute ``name`` of its ``of`` object (what the tests and tools look at)."""
    return property(lambda self: getattr(getattr(self, of), name))


# ---- shared checks and the read-back ---------------------------------------------------------------------------------------------
def is_int_in(v, lo, hi=None):
    """``v`` is an integer (no bool, no float) with lo <= v (<= hi)."""
    return not isinstance(v, bool) and isinstance(v, (int, np.integer)) and lo <= v and (hi is None or v <= hi)


def check_unit(who, name, v):
    """Raises unless the threshold ``v`` lies in (0, 1] (NaN fails too)."""
    if not 0.0 < v <= 1.0:
        raise ValueError("{}{} must lie in (0, 1]".format(who, name))


def as_mask(m):
    """A truth mask as int32 (the kernels test != 0: int32 goes as it is)."""
    return m if m.dtype == torch.int32 else (m != 0).to(torch.int32)


def check_shapes(fn, items):
    """Raises for the first of ``items`` = (name, tensor, shape) of a ``truth`` dict that has another shape."""
    for name, t, shp in items:
        if tuple(t.shape) != shp:
            raise ValueError(fn + "truth[{!r}] of shape {} given, {} expected".format(name, tuple(t.shape), list(shp)))


def read_back(core, tensors, zero=False):
    """Host copies of the device tensors {name: tensor}, cloned on the core's stream (joined with the caller's on the way in and
    out); ``zero``: they start again from zero afterwards."""
    with torch.cuda.device(core.device):
        core._join_in()
        with core.on_stream():
            got = {n: t.clone() for n, t in tensors.items()}
            if zero:
                for t in tensors.values():
                    t.zero_()
        core._join_out()
        return {n: t.cpu() for n, t in got.items()}


def _columns(table, names):
    """The last axis of an accumulator table by name, copies."""
    return {n: table[..., i].clone() for i, n in enumerate(names)}


def _ratio(a, b):
    return float(a) / b if b else float("nan")


def hota_figures(ints, floats):
    """The ratios of HOTA (include/sqair_hip.h: sqair_set_hota, point 6) from one set of totals, ``ints`` [19, 4] = (tp, fn, fp, loc)
    and ``floats`` [19, 3] = (ass, assre, asspr): ``hota_alpha``, ``deta_alpha``, ``assa_alpha`` [19] float64 arrays, their means over
    the thresholds ``hota``, ``deta``, ``assa``, ``detre``, ``detpr``, ``assre``, ``asspr``, ``loca``, and ``hota0`` / ``loca0``, the
    figures at alpha = 0.05.  A ratio without a denominator is NaN, and so is a mean over one.  With leading axes ([..., 19, 4] and
    [..., 19, 3]) a list of such dicts, one per set, computed together."""
    ints, floats = np.asarray(ints, np.float64), np.asarray(floats, np.float64)
    if ints.ndim > 2:
        lead = ints.shape[:-2]
        return _hota_figures(ints.reshape((-1,) + ints.shape[-2:]), floats.reshape((-1,) + floats.shape[-2:]), int(np.prod(lead)))
    return _hota_figures(ints[None], floats[None], 1)[0]


def _hota_figures(ints, floats, n_sets):
    tp, fn, fp, loc = (ints[..., i] for i in range(4))
    div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1.0), np.nan)
    per = dict(deta=div(tp, tp + fn + fp), detre=div(tp, tp + fn), detpr=div(tp, tp + fp), assa=div(floats[..., 0], tp),
               assre=div(floats[..., 1], tp), asspr=div(floats[..., 2], tp), loca=div(loc / 1048576.0, tp))
    per["hota"] = np.sqrt(per["deta"] * per["assa"])
    mean = {n: v.mean(-1).tolist() for n, v in per.items()}
    out = []
    for i in range(n_sets):
        res = {n: v[i] for n, v in mean.items()}
        res.update(hota_alpha=per["hota"][i], deta_alpha=per["deta"][i], assa_alpha=per["assa"][i], hota0=float(per["hota"][i, 0]),
                   loca0=float(per["loca"][i, 0]))
        out.append(res)
    return out


def track_log_views(got):
    """What ``SqairStream.track_log`` returns, formed on the host from the solve's outputs read back (include/sqair_hip.h:
    sqair_lane_tracklog_smooth; host tensors {name: tensor} by _capi.TRACKLOG_OUT_FIELDS): ``track_id``, ``n_tracks``, ``len0``,
    ``frame_index``, ``state`` and ``size`` as they are, and for each of ``smooth`` and ``filtered`` a dict of ``centre``, ``velocity``,
    ``sigma`` = sqrt(max(Ppp, 0)) [lag, B, C, 2] = (y, x) and ``box`` [lag, B, C, 4] = (centre - size / 2, size)."""
    res = {n: got[n] for n in ("track_id", "n_tracks", "len0", "frame_index", "state", "size")}
    for name, field in (("smooth", "smooth"), ("filtered", "filt")):
        kf = _columns(got[field], _capi.MOTION_STATE)
        res[name] = dict(centre=kf["p"], velocity=kf["v"], sigma=kf["Ppp"].clamp(min=0.0).sqrt(),
                         box=torch.cat([kf["p"] - 0.5 * got["size"], got["size"]], -1))
    return res


def ring_runs(n, T, L):
    """Where the T frames of a step go in a ring of L positions that has taken n frames: [(lo, hi, at)], frames lo..hi-1 of the step
    to positions at.. -- frame t at (n + t) mod L, as contiguous runs; of a step longer than the ring only the last L frames stay."""
    runs, t = [], max(0, T - L)
    while t < T:
        at = (n + t) % L
        m = min(T - t, L - at)
        runs.append((t, t + m, at))
        t += m
    return runs


def ring_window(ring, n, lag):
    """The last ``lag`` positions of a ring tensor [L, ...] that has taken n frames, in window order (oldest first): window frame f
    is stream frame n - lag + f at position (n - lag + f) mod L.  A new tensor; frames before the ring existed (n - lag + f < 0) hold
    whatever the position holds -- the caller invalidates them."""
    L = ring.shape[0]
    start = (n - lag) % L
    if start + lag <= L:
        return ring[start:start + lag].clone()
    return torch.cat([ring[start:], ring[:start + lag - L]])


def track_log_score(got):
    """``track_log(score=True)``'s ``log["score"]``, formed on the host from the scorer's outputs read back (include/sqair_hip.h:
    sqair_lane_tracklog_score; host tensors by _capi.tracklog_score_shapes): per view name of _capi.TRACKLOG_SCORE_VIEWS a dict of
    the per-lane counters [B] int64 and sums [B] float64 by name, ``assign`` [B, G], ``match`` and ``match_iou`` [lag, B, G], and
    pooled over the lanes, formed from the counters as ``score()`` and ``idf_score()`` form theirs and NaN where a denominator is 0:
    ``mota`` = 1 - (fn + fp + idsw) / truth, ``motp`` = iou_sum / tp, ``idf1`` = 2 idtp / (2 idtp + idfp + idfn), ``idp`` = idtp /
    (idtp + idfp), ``idr`` = idtp / (idtp + idfn), ``mean_err`` = err_sum / tp (pixels), ``nees`` = nees_sum / nees_n (2 for an
    honest sigma), and over the filled gaps ``gap_err`` = gap_err_sum / gap_tp, ``gap_nees`` = gap_nees_sum / gap_nees_n and
    ``gap_precision`` = gap_tp / (gap_tp + gap_fp)."""
    res = {}
    for v, name in enumerate(_capi.TRACKLOG_SCORE_VIEWS):
        r = _columns(got["counts"][:, v], _capi.TRACKLOG_SCORE_COUNTS)
        r.update(_columns(got["sums"][:, v], _capi.TRACKLOG_SCORE_SUMS))
        tot = {n: (float if n in _capi.TRACKLOG_SCORE_SUMS else int)(t.sum()) for n, t in r.items()}
        r.update(assign=got["assign"][v], match=got["match"][v], match_iou=got["match_iou"][v])
        r["mota"] = 1.0 - _ratio(tot["fn"] + tot["fp"] + tot["idsw"], tot["truth"])
        r["motp"] = _ratio(tot["iou_sum"], tot["tp"])
        r["idf1"] = _ratio(2 * tot["idtp"], 2 * tot["idtp"] + tot["idfp"] + tot["idfn"])
        r["idp"] = _ratio(tot["idtp"], tot["idtp"] + tot["idfp"])
        r["idr"] = _ratio(tot["idtp"], tot["idtp"] + tot["idfn"])
        r["mean_err"] = _ratio(tot["err_sum"], tot["tp"])
        r["nees"] = _ratio(tot["nees_sum"], tot["nees_n"])
        r["gap_err"] = _ratio(tot["gap_err_sum"], tot["gap_tp"])
        r["gap_nees"] = _ratio(tot["gap_nees_sum"], tot["gap_nees_n"])
        r["gap_precision"] = _ratio(tot["gap_tp"], tot["gap_tp"] + tot["gap_fp"])
        res[name] = r
    return res


def track_log_fit(got, q_grid, r_grid):
    """``SqairStream.track_log_fit``'s result, formed on the host from the fit's outputs read back (include/sqair_hip.h:
    sqair_lane_tracklog_fit; ``got``: host tensors or arrays ``counts`` [B, Q, R, 3], ``sums`` [B, Q, R, 4] and optionally ``innov``):
    ``q_grid`` [Q] and ``r_grid`` [R] float64; pooled over the lanes, per grid node [Q, R]: ``n``, ``n_gap``, ``skipped`` int64, ``nll`` =
    1/2 (n ln 2 pi + lns_sum + nis_sum) (nats), ``mean_nis`` = nis_sum / n (1 for an honest filter) and ``gap_mean_nis`` =
    gap_nis_sum / n_gap, the same over the first innovations behind a gap, NaN where the denominator is 0; per lane [B, Q, R] the
    same under ``lane_n``, ``lane_n_gap``, ``lane_skipped``, ``lane_nll``, ``lane_mean_nis``, ``lane_gap_mean_nis``.  ``node`` = (iq, ir),
    the first node in index order of minimal pooled ``nll``, ``q`` and ``r`` its values: the maximum-likelihood fit on the grid;
    ``at_edge``: the node lies on the grid's border along an axis of more than one value -- the minimum may lie outside, fit again
    with a grid moved there.  ``lane_q``, ``lane_r`` [B]: the same per lane.  Without a counted term (pooled, or of a lane) there is
    no fit: ``node`` is None, the values NaN, ``at_edge`` False.  Nodes are compared as they stand: where ``skipped`` differs between
    nodes, so does the number of terms.  ``innov`` [lag, B, C, 2, 2], (y, S) of node (0, 0) per (frame, lane, column, axis), if
    it was asked for."""
    counts = np.asarray(torch.as_tensor(got["counts"]).numpy(), np.int64)
    sums = np.asarray(torch.as_tensor(got["sums"]).numpy(), np.float64)
    qg, rg = np.asarray(q_grid, np.float64).reshape(-1), np.asarray(r_grid, np.float64).reshape(-1)
    if counts.shape[1:3] != (len(qg), len(rg)) or sums.shape[:3] != counts.shape[:3]:
        raise ValueError("lane.track_log_fit: counts {} and sums {} given for a {} x {} grid".format(
            tuple(counts.shape), tuple(sums.shape), len(qg), len(rg)))

    def figures(c, s):
        n, n_gap = c[..., 0], c[..., 1]
        div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1), np.nan)
        return dict(n=n, n_gap=n_gap, skipped=c[..., 2], nll=0.5 * (n * np.log(2.0 * np.pi) + s[..., 1] + s[..., 0]),
                    mean_nis=div(s[..., 0], n), gap_mean_nis=div(s[..., 2], n_gap))

    def best(f):
        node = np.unravel_index(int(np.argmin(f["nll"])), f["nll"].shape)   # (argmin: the first of equal minima in index order)
        return tuple(int(i) for i in node) if f["n"][node] > 0 else None
    pooled, lanes = figures(counts.sum(0), sums.sum(0)), figures(counts, sums)
    res = dict(q_grid=torch.from_numpy(qg.copy()), r_grid=torch.from_numpy(rg.copy()))
    res.update({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in pooled.items()})
    res.update({"lane_" + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in lanes.items()})
    node = res["node"] = best(pooled)
    res["q"], res["r"] = (float(qg[node[0]]), float(rg[node[1]])) if node else (float("nan"), float("nan"))
    res["at_edge"] = bool(node) and any(m > 1 and i in (0, m - 1) for i, m in zip(node, (len(qg), len(rg))))
    lane_nodes = [best({k: v[b] for k, v in lanes.items()}) for b in range(counts.shape[0])]
    res["lane_q"] = torch.tensor([qg[nd[0]] if nd else float("nan") for nd in lane_nodes], dtype=torch.float64)
    res["lane_r"] = torch.tensor([rg[nd[1]] if nd else float("nan") for nd in lane_nodes], dtype=torch.float64)
    if got.get("innov") is not None:
        res["innov"] = torch.as_tensor(got["innov"])
    return res


def mot_rows(log, lane):
    """The MOTChallenge rows (frame, id, x, y, w, h) of lane ``lane`` of a ``track_log()`` result: one row per (frame, track) whose
    ``state`` is 1 (seen) or 2 (a gap the smoother filled), from the smoothed boxes, ordered by frame, then by id; ``frame`` is the
    absolute frame number ``frame_index``, x and y the box's left and top edge.  A float64 array [rows, 6]."""
    state = np.asarray(log["state"])[:, lane]
    box = np.asarray(log["smooth"]["box"], np.float64)[:, lane]
    frame, ids = np.asarray(log["frame_index"])[:, lane], np.asarray(log["track_id"])[lane]
    rows = [(frame[f], ids[c], box[f, c, 1], box[f, c, 0], box[f, c, 3], box[f, c, 2])
            for f in range(state.shape[0]) for c in range(state.shape[1]) if state[f, c] in (1, 2)]
    return np.asarray(rows, np.float64).reshape(-1, 6)


def field_views(shapes, int_fields, device):
    """The fields {name: shape} as views of ONE float32 allocation, each 16-byte aligned (``int_fields``: viewed as int32), so that
    they are copied out with one launch instead of one per field.  Returns (flat, views): views(flat or a clone of it) -> {name: view}."""
    sizes = {n: int(np.prod(shp)) for n, shp in shapes.items()}
    offs = dict(zip(sizes, np.cumsum([0] + [(s + 3) // 4 * 4 for s in sizes.values()]).tolist()))
    flat = torch.zeros(offs[list(sizes)[-1]] + sizes[list(sizes)[-1]], dtype=torch.float32, device=device)
    return flat, lambda flat: {n: (flat[offs[n]:offs[n] + sizes[n]].view(torch.int32) if n in int_fields
                                   else flat[offs[n]:offs[n] + sizes[n]]).view(shapes[n]) for n in shapes}


def zeros_of(owner, shapes, device):
    """{name: zeros of its shape} for pointer fields of the struct ``owner`` of include/sqair_hip.h (or pointer parameters of the
    function ``owner``), each in the element type the header declares it with."""
    return {n: torch.zeros(shp, dtype=getattr(torch, _capi.field_dtype(owner, n)), device=device) for n, shp in shapes.items()}


# ---- the resident stack: estimate, layers, identity, score -----------------------------------------------------------------------
class LaneAnswers(object):
    """The lane answers a stream's steps fill.  The constructor only checks its keyword group (no core, no device: it runs before the
    stream touches either); ``register`` allocates the buffers and registers them on the core's handle.  ``flat`` / ``views``: ONE
    allocation and its views by field, ``est`` (field_views) -- everything a step copies out as ``out["lane"]``; ``score_buf`` and
    ``ident_buf``: the score's truth, accumulators and identity memory, the identity's track table and counters; ``tracklog_buf``:
    the track log's ring of every lane, ``truth_ring`` (with ``tracklog_truth``) the truth of the last L stepped frames beside it and
    ``ring_frames`` the frames it has taken; ``idf_buf``: the
    IDF1 table of every lane's open clip and the totals over the closed ones; ``hota_buf``: the HOTA log of every lane's open clip
    and its totals."""

    def __init__(self, who, estimate, estimate_iou, estimate_canvas, estimate_layers, layers_cover_min, score, score_iou, score_truth,
                 identity, identity_iou, identity_tracks, identity_max_age, identity_reid_dist, identity_reid_what, identity_appearance,
                 score_ids, score_idf=False, score_idf_ids=32, score_match="greedy", identity_match="greedy", score_hota=False,
                 score_hota_ids=32, score_hota_frames=256, motion=False, motion_q=0.25, motion_r=1.0, motion_v0=16.0, motion_gate=3.0,
                 motion_nis=False, tracklog=None, tracklog_tracks=16, tracklog_truth=None):
        self.step_fn, who = who + ".step: ", who + ": "

        def bad(why):
            raise ValueError(who + why)
        self.estimate_iou = float(estimate_iou)
        if estimate:
            check_unit(who, "estimate_iou", self.estimate_iou)
        if estimate_canvas and not estimate:
            bad("estimate_canvas is for a stream with estimate=True")
        if estimate_layers and not estimate:
            bad("estimate_layers is for a stream with estimate=True")
        self.cover_min = float(layers_cover_min)
        if estimate_layers:
            check_unit(who, "layers_cover_min", self.cover_min)
        if score and not estimate:
            bad("score is for a stream with estimate=True")
        self.score_iou = float(score_iou)
        if score:
            check_unit(who, "score_iou", self.score_iou)
        if score and score_truth is not None and not is_int_in(score_truth, 1, _capi.SCORE_MAX_TRUTH):
            bad("score_truth must be an integer in [1, {}]".format(_capi.SCORE_MAX_TRUTH))
        if identity and not estimate:
            bad("identity is for a stream with estimate=True")
        self.identity_iou, self.reid_dist, self.reid_what = float(identity_iou), float(identity_reid_dist), float(identity_reid_what)
        if identity:
            check_unit(who, "identity_iou", self.identity_iou)
        self._tracks_text = "identity_tracks must be an integer in [n_steps_per_image, {}]".format(_capi.IDENT_MAX_TRACKS)
        if identity and identity_tracks is not None and not is_int_in(identity_tracks, 1, _capi.IDENT_MAX_TRACKS):
            bad(self._tracks_text)
        if identity and not is_int_in(identity_max_age, 0):
            bad("identity_max_age must be an integer >= 0")
        if identity and not self.reid_dist >= 0.0:   # (NaN fails too)
            bad("identity_reid_dist must be >= 0")
        if identity and not self.reid_what > 0.0:   # (NaN fails too)
            bad("identity_reid_what must lie in (0, +inf]")
        if motion and not identity:
            bad("motion is for a stream with identity=True")
        if motion_nis and not motion:
            bad("motion_nis is for a stream with motion=True")
        self.motion_scalars = dict(q=float(motion_q), r=float(motion_r), v0_var=float(motion_v0), gate=float(motion_gate))
        for name, v in zip(("motion_q", "motion_r", "motion_v0", "motion_gate"), self.motion_scalars.values()):
            if motion and not 0.0 < v < float("inf"):   # (NaN fails too)
                bad(name + " must be finite and > 0")
        self.motion, self.motion_nis = bool(motion), bool(motion_nis)
        if tracklog is not None and not identity:
            bad("tracklog is for a stream with identity=True")
        if tracklog is not None and not is_int_in(tracklog, 1, _capi.TRACKLOG_MAX_FRAMES):
            bad("tracklog must be an integer in [1, {}]".format(_capi.TRACKLOG_MAX_FRAMES))
        if tracklog is not None and not is_int_in(tracklog_tracks, 1, _capi.TRACKLOG_MAX_TRACKS):
            bad("tracklog_tracks must be an integer in [1, {}]".format(_capi.TRACKLOG_MAX_TRACKS))
        self.tracklog = tracklog is not None
        self.log_L, self.log_C = (int(tracklog), int(tracklog_tracks)) if self.tracklog else (0, 0)
        if tracklog_truth is not None and not self.tracklog:
            bad("tracklog_truth is for a stream with tracklog=L")
        if tracklog_truth is not None and not is_int_in(tracklog_truth, 1, _capi.SCORE_MAX_TRUTH):
            bad("tracklog_truth must be an integer in [1, {}]".format(_capi.SCORE_MAX_TRUTH))
        self._truth_text = "tracklog_truth must equal score_truth: a step's truth feeds the score and the log's truth ring alike"
        if tracklog_truth is not None and score and score_truth is not None and int(score_truth) != int(tracklog_truth):
            bad(self._truth_text)
        self.log_G = 0 if tracklog_truth is None else int(tracklog_truth)   # truth slots of the log's truth ring; 0: none is kept
        if score_ids not in ("row", "lane"):
            bad("score_ids must be 'row' or 'lane'")
        if score_ids == "lane" and not (score and identity):
            bad("score_ids='lane' is for a stream with score=True and identity=True")
        if score_idf and not score:
            bad("score_idf is for a stream with score=True")
        if score_idf and not is_int_in(score_idf_ids, 1, _capi.IDF_MAX_IDS):
            bad("score_idf_ids must be an integer in [1, {}]".format(_capi.IDF_MAX_IDS))
        if score_hota and not score:
            bad("score_hota is for a stream with score=True")
        if score_hota and not is_int_in(score_hota_ids, 1, _capi.HOTA_MAX_IDS):
            bad("score_hota_ids must be an integer in [1, {}]".format(_capi.HOTA_MAX_IDS))
        if score_hota and not is_int_in(score_hota_frames, 1, _capi.HOTA_MAX_FRAMES):
            bad("score_hota_frames must be an integer in [1, {}]".format(_capi.HOTA_MAX_FRAMES))
        for name, v, flag, needs in (("score_match", score_match, score, "score=True"),
                                     ("identity_match", identity_match, identity, "identity=True")):
            if v not in MATCH_MODES:
                bad("{} must be 'greedy' or 'optimal'".format(name))
            if v == "optimal" and not flag:
                bad("{}='optimal' is for a stream with {}".format(name, needs))
        self.score_match, self.identity_match = MATCH_MODES.index(score_match), MATCH_MODES.index(identity_match)
        self.idf, self.P = bool(score_idf), int(score_idf_ids) if score_idf else 0
        self.hota = bool(score_hota)
        self.hota_P, self.hota_L = (int(score_hota_ids), int(score_hota_frames)) if score_hota else (0, 0)
        self.who = who
        self.estimate, self.canvas, self.layers = bool(estimate), bool(estimate_canvas), bool(estimate_layers)
        self.scored, self.identified, self.appearance = bool(score), bool(identity), bool(identity_appearance)
        self._truth_slots, self._tracks, self.max_age, self.score_ids = score_truth, identity_tracks, identity_max_age, score_ids
        self.G = self.M = 0   # truth slots, track entries per lane (size)

    def size(self, core):
        """``G`` and ``M`` for the core's N slots: the last check, and the only one that needs the core (its handle is not touched)."""
        if self.scored:
            self.G = core.N if self._truth_slots is None else int(self._truth_slots)
            if self.log_G and self.log_G != self.G:   # (score_truth defaulted to the core's N)
                raise ValueError(self.who + self._truth_text)
        if self.identified:
            self.M = min(_capi.IDENT_MAX_TRACKS, 2 * core.N) if self._tracks is None else int(self._tracks)
            if not core.N <= self.M:
                raise ValueError(self.who + self._tracks_text)

    def register(self, core, log_w, T, B):
        """Allocates the buffers and registers them on the handle: the estimate (``log_w``: the carried log weights -- after SMC, so
        that they are the resampler's accumulator), then layers, score, identity, score_ids; first of all the matching modes, a
        plain setting of the handle that the passes read (sqair_set_lane_match; its traj_link is ``TrajScores.launch``'s, per call)."""
        self.core, self.T, self.B = core, T, B
        core.check(core.lib.sqair_set_lane_match(core.handle, self.score_match, self.identity_match, 0), "sqair_set_lane_match")
        if not self.estimate:
            return
        lib, h, G, K, N = core.lib, core.handle, self.G, core.K, core.N
        shapes = _capi.estimate_shapes(T, B, K, N, core.nw, (core.H, core.W) if self.canvas else None)
        ints = _capi.ESTIMATE_INT_FIELDS
        if self.layers:
            shapes.update(_capi.layers_shapes(T, B, K, N, (core.H, core.W)))
            ints = ints + _capi.LAYERS_INT_FIELDS
        if self.scored:
            shapes.update(_capi.score_shapes(T, B, G))
            ints = ints + _capi.SCORE_INT_FIELDS
        if self.identified:
            shapes.update(_capi.identity_shapes(T, B, N))
            ints = ints + tuple(_capi.IDENT_LANE_NAMES[n] for n in _capi.IDENT_INT_FIELDS)
        if self.motion:
            shapes.update({n: s for n, s in _capi.motion_shapes(T, B, N).items() if n != "nis" or self.motion_nis})
        self.flat, self.views = field_views(shapes, ints, core.device)
        est = self.est = self.views(self.flat)
        sync = torch.cuda.current_stream(core.device).synchronize   # (a buffer's initial values are in place before a pass reads it)
        c_est = _capi.SqairLaneEstimate(iou_min=self.estimate_iou, log_w=log_w.data_ptr(),
                                        **{n: t.data_ptr() for n, t in est.items() if n in _capi.ESTIMATE_FIELDS})
        sync()
        core.check(lib.sqair_set_estimate(h, C.byref(c_est), T, B), "sqair_set_estimate")
        if self.layers:
            lay = _capi.SqairLaneLayers(cover_min=self.cover_min, **{n: est[n].data_ptr() for n in _capi.LAYERS_FIELDS})
            core.check(lib.sqair_set_layers(h, C.byref(lay), T, B), "sqair_set_layers")
        if self.scored:   # the truth of a step, the accumulators and the identity memory
            self.score_buf = zeros_of("SqairLaneScore", dict(truth_box=(T, B, G, 4), truth_present=(T, B, G), truth_valid=(T, B),
                                                             counts=(B, len(_capi.SCORE_COUNTS)), iou_sum=(B,), last_id=(B, G)), core.device)
            self.score_buf["last_id"].fill_(-1)
            self._valid_is_zero = True
            sc = _capi.SqairLaneScore(iou_min=self.score_iou, G=G, **{n: t.data_ptr() for n, t in self.score_buf.items()},
                                      **{n: est[n].data_ptr() for n in _capi.SCORE_FIELDS})
            sync()
            core.check(lib.sqair_set_score(h, C.byref(sc), T, B), "sqair_set_score")
        if self.identified:   # the track table of every lane and the counters
            shapes = _capi.identity_memory_shapes(B, self.M, core.nw)
            if not self.appearance:
                del shapes["trk_what"]
            self.ident_buf = zeros_of("SqairLaneIdentity", shapes, core.device)
            self.ident_buf["trk_id"].fill_(-1)
            idt = _capi.SqairLaneIdentity(iou_min=self.identity_iou, reid_dist=self.reid_dist, reid_what=self.reid_what, M=self.M,
                                          max_age=int(self.max_age), **{n: t.data_ptr() for n, t in self.ident_buf.items()},
                                          **{n: est[_capi.IDENT_LANE_NAMES[n]].data_ptr() for n in _capi.IDENT_FIELDS})
            sync()
            core.check(lib.sqair_set_identity(h, C.byref(idt), T, B), "sqair_set_identity")
            if self.motion:   # the filter's state beside the track table: the identity's node in its motion instantiation
                self.ident_buf.update(zeros_of("SqairLaneMotion", _capi.motion_memory_shapes(B, self.M), core.device))
                mo = _capi.SqairLaneMotion(trk_kf=self.ident_buf["trk_kf"].data_ptr(), **self.motion_scalars,
                                           **{n: est[n].data_ptr() for n in _capi.MOTION_FIELDS if n in est})
                sync()
                core.check(lib.sqair_set_motion(h, C.byref(mo), T, B), "sqair_set_motion")
            if self.tracklog:   # the ring of every lane beside the track table: one more node, right behind the identity's
                self.tracklog_buf = zeros_of("SqairLaneTrackLog", _capi.tracklog_shapes(B, self.log_L, N), core.device)
                self._log_c = _capi.SqairLaneTrackLog(L=self.log_L, **{n: t.data_ptr() for n, t in self.tracklog_buf.items()})
                self._log_out = {}   # the solve's outputs and scratch of the LAST lag asked for
                if self.log_G:   # the truth of the last L stepped frames beside the log: written by copies, read by track_log(score=True)
                    self.truth_ring = zeros_of("SqairTrackLogTruth", _capi.tracklog_truth_shapes(self.log_L, B, self.log_G), core.device)
                    self.ring_frames = 0   # frames stepped since the ring was made: frame t of a step goes to (ring_frames + t) mod L
                sync()
                core.check(lib.sqair_set_tracklog(h, C.byref(self._log_c), T, B), "sqair_set_tracklog")
            if self.score_ids == "lane":
                core.check(lib.sqair_set_score_ids(h, 1), "sqair_set_score_ids")
        if self.idf:   # the overlap table of every lane's open clip, the totals over the closed ones, and what a solve writes
            self.idf_buf = zeros_of("SqairLaneIdf", _capi.idf_shapes(B, G, self.P), core.device)
            self.idf_buf["col_id"].fill_(-1)
            self._idf_c = _capi.SqairLaneIdf(P=self.P, **{n: t.data_ptr() for n, t in self.idf_buf.items()})
            self._idf_out = zeros_of("sqair_lane_idf_solve", dict(open=(B, len(_capi.IDF_TOTALS)), assign=(B, G), close=(B,)), core.device)
            sync()
            core.check(lib.sqair_set_idf(h, C.byref(self._idf_c), T, B), "sqair_set_idf")
        if self.hota:   # the clip log of every lane, the totals over the closed clips, and what a solve writes
            self.hota_buf = zeros_of("SqairLaneHota", _capi.hota_shapes(B, G, N, self.hota_P, self.hota_L), core.device)
            self.hota_buf["col_id"].fill_(-1)
            self._hota_c = _capi.SqairLaneHota(P=self.hota_P, L=self.hota_L, **{n: t.data_ptr() for n, t in self.hota_buf.items()})
            shapes = _capi.hota_solve_shapes(B, G, self.hota_L)
            del shapes["match"]
            self._hota_out = zeros_of("sqair_lane_hota_solve", shapes, core.device)
            sync()
            core.check(lib.sqair_set_hota(h, C.byref(self._hota_c), T, B), "sqair_set_hota")

    # ---- per step ------------------------------------------------------------------------------------------------------------
    def check_truth(self, truth):
        """``truth`` of a step as (box float32 [T', B, G, 4], present int32 [T', B, G], valid int32 [T', B]) (None: no truth)."""
        if truth is None:
            return None
        fn = self.step_fn
        if not (self.scored or self.log_G):
            raise ValueError(fn + "truth is for a stream with score=True")
        if not isinstance(truth, dict) or "box" not in truth or "present" not in truth or set(truth) - {"box", "present", "valid"}:
            raise ValueError(fn + "truth must be a dict with box, present and optionally valid")
        T, B, G = self.T, self.B, self.G if self.scored else self.log_G
        box = torch.as_tensor(truth["box"]).to(torch.float32)
        present = torch.as_tensor(truth["present"])
        valid = truth.get("valid")
        valid = torch.ones((T, B), dtype=torch.int32) if valid is None else torch.as_tensor(valid)
        if T == 1 and box.dim() == 3:
            box, present, valid = box[None], present[None], (valid[None] if valid.dim() == 1 else valid)
        check_shapes(fn, (("box", box, (T, B, G, 4)), ("present", present, (T, B, G)), ("valid", valid, (T, B))))
        return box, as_mask(present), as_mask(valid)

    def feed_truth(self, truth):
        """A step's checked truth into the score's own buffers, on the current stream (as the mask of a stream with missing frames:
        the kernel reads the stream's buffers, so one graph serves every step); without one ``truth_valid`` is zeroed once.  A
        stream with ``tracklog_truth`` then writes the step's frames into the log's truth ring, frame t at (ring_frames + t) mod L --
        from the score's buffers where there is a score, so the truth is uploaded once --, or zeroes ``truth_valid`` there."""
        names = ("truth_box", "truth_present", "truth_valid")
        if self.scored:
            if truth is not None:
                for n, t in zip(names, truth):
                    self.score_buf[n].copy_(t, non_blocking=True)
            elif not self._valid_is_zero:
                self.score_buf["truth_valid"].zero_()
            self._valid_is_zero = truth is None
        if self.log_G:
            src = None if truth is None else self.score_buf if self.scored else dict(zip(names, truth))
            for lo, hi, at in ring_runs(self.ring_frames, self.T, self.log_L):
                if src is None:
                    self.truth_ring["truth_valid"][at:at + hi - lo].zero_()
                else:
                    for n in names:
                        self.truth_ring[n][at:at + hi - lo].copy_(src[n][lo:hi], non_blocking=True)
            self.ring_frames += self.T

    def copy_out(self):
        """``out["lane"]`` of the step just run: views of one clone."""
        return self.views(self.flat.clone())

    def reset(self, lanes, on_core_stream):
        """The follow-ups of a stream's ``reset(lanes)`` (``lanes`` checked and distinct; ``on_core_stream``: the carried state's context):
        the score forgets those lanes' identities (``last_id``) and keeps their counters; the identity frees their track entries
        (``trk_id`` = -1) and keeps their ``next_id``, and a stream with ``tracklog`` zeroes their ``count``.  Before either, a stream with ``score_idf`` closes those lanes' clips: one solve
        with their mask, their figures into the totals, their tables freed; a stream with ``score_hota`` does the same with its log."""
        if lanes and (self.scored or self.identified):
            with on_core_stream():
                if self.idf:
                    close = self._idf_out["close"]
                    close.zero_()
                    close[torch.as_tensor(lanes, device=close.device)] = 1
                    self._solve(close)
                if self.hota:
                    close = self._hota_out["close"]
                    close.zero_()
                    close[torch.as_tensor(lanes, device=close.device)] = 1
                    self._hota_solve(close)
                for j in lanes:
                    if self.scored:
                        self.score_buf["last_id"][j].fill_(-1)
                    if self.identified:
                        self.ident_buf["trk_id"][j].fill_(-1)
                    if self.tracklog:   # (a new clip starts an empty log; ids are never reused within a lane)
                        self.tracklog_buf["count"][j].zero_()

    # ---- read-outs -----------------------------------------------------------------------------------------------------------
    def score(self, reset=False):
        if not self.scored:
            raise ValueError("SqairStream.score: the stream keeps no score (SqairStream(..., estimate=True, score=True))")
        got = read_back(self.core, {n: self.score_buf[n] for n in ("counts", "iou_sum")}, zero=reset)
        res = _columns(got["counts"], _capi.SCORE_COUNTS)
        tot = {n: int(v.sum()) for n, v in res.items()}
        res["iou_sum"] = got["iou_sum"]
        res["mota"] = 1.0 - _ratio(tot["fn"] + tot["fp"] + tot["idsw"], tot["truth"])
        res["motp"] = _ratio(float(got["iou_sum"].sum()), tot["tp"])
        res["count_accuracy"] = _ratio(tot["count_hit"], tot["frames"])
        return res

    def _solve(self, close=None):
        """One solve on the current stream (include/sqair_hip.h: sqair_lane_idf_solve) into ``_idf_out``; ``close``: the device mask
        [B] of the lanes whose clip ends."""
        core, o = self.core, self._idf_out
        core.check(core.lib.sqair_lane_idf_solve(core.handle, C.byref(self._idf_c), self.G, self.B,
                                                 None if close is None else close.data_ptr(), o["open"].data_ptr(), o["assign"].data_ptr(),
                                                 core._stream()), "sqair_lane_idf_solve")

    def idf_score(self, reset=False):
        if not self.idf:
            raise ValueError("SqairStream.idf_score: the stream keeps no IDF1 table (SqairStream(..., estimate=True, score=True, "
                             "score_idf=True))")
        core, buf = self.core, self.idf_buf
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                self._solve()
                got = {n: t.clone() for n, t in (("totals", buf["totals"]), ("open", self._idf_out["open"]), ("assign", self._idf_out["assign"]))}
                if reset:   # the totals from zero, every table free (what a close leaves, without counting the clip)
                    buf["col_id"].fill_(-1)
                    for n in ("totals", "row_frames", "matched", "frag", "trk_state", "extra_frames", "frames"):
                        buf[n].zero_()
            core._join_out()
        got = {n: t.cpu() for n, t in got.items()}
        res = _columns(got["totals"] + got["open"], _capi.IDF_TOTALS)
        tot = {n: int(v.sum()) for n, v in res.items()}
        res["assign"] = got["assign"]
        res["idf1"] = _ratio(2 * tot["idtp"], 2 * tot["idtp"] + tot["idfp"] + tot["idfn"])
        res["idp"] = _ratio(tot["idtp"], tot["idtp"] + tot["idfp"])
        res["idr"] = _ratio(tot["idtp"], tot["idtp"] + tot["idfn"])
        res["mt_rate"] = _ratio(tot["mt"], tot["trajectories"])
        res["ml_rate"] = _ratio(tot["ml"], tot["trajectories"])
        res["frag_per_lane"], res["frag"] = res["frag"], tot["frag"]
        res["exact"] = tot["overflow_ids"] == 0
        return res

    def _hota_solve(self, close=None):
        """One solve on the current stream (include/sqair_hip.h: sqair_lane_hota_solve) into ``_hota_out``; ``close``: the device mask
        [B] of the lanes whose clip ends."""
        core, o = self.core, self._hota_out
        core.check(core.lib.sqair_lane_hota_solve(core.handle, C.byref(self._hota_c), self.G, core.N, self.B,
                                                  None if close is None else close.data_ptr(), o["open_i"].data_ptr(),
                                                  o["open_f"].data_ptr(), o["open_c"].data_ptr(), None, core._stream()),
                   "sqair_lane_hota_solve")

    def hota_score(self, reset=False):
        if not self.hota:
            raise ValueError("SqairStream.hota_score: the stream keeps no HOTA log (SqairStream(..., estimate=True, score=True, "
                             "score_hota=True))")
        core, buf = self.core, self.hota_buf
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                self._hota_solve()
                got = {n: (buf["totals" + n[4:]] + self._hota_out[n]) for n in ("open_i", "open_f", "open_c")}
                if reset:   # the totals from zero, every lane free (what a close leaves, without counting the clip)
                    buf["col_id"].fill_(-1)
                    for n in _capi.HOTA_TOTALS + ("frames", "dropped_frames"):
                        buf[n].zero_()
            core._join_out()
        got = {n: t.cpu() for n, t in got.items()}
        res = _columns(got["open_i"], _capi.HOTA_INT)
        res.update(_columns(got["open_f"], [n + "_sum" for n in _capi.HOTA_FLOAT]))      # (assre, asspr: the ratios' means, below)
        res.update(_columns(got["open_c"], _capi.HOTA_CLIP))
        ints, floats = got["open_i"].numpy(), got["open_f"].numpy()      # (the lanes and, last, their sum: one set of ratios each)
        sets = hota_figures(np.concatenate([ints, ints.sum(0)[None]]), np.concatenate([floats, floats.sum(0)[None]]))
        res["lanes"] = sets[:-1]
        res.update(sets[-1])
        res["exact"] = int(res["dropped_frames"].sum()) == 0 and int(res["overflow_ids"].sum()) == 0
        return res

    def _check_log_call(self, fn, lag, q, r, v0):
        """What ``track_log`` and ``track_log_fit`` check alike: (lag, the solve's scalars {q, r, v0}, None = the stream's)."""
        if not self.tracklog:
            raise ValueError("SqairStream.{}: the stream keeps no track log (SqairStream(..., estimate=True, identity=True, "
                             "tracklog=L))".format(fn))
        lag = self.log_L if lag is None else lag
        if not is_int_in(lag, 1, self.log_L):
            raise ValueError("SqairStream.{}: lag must be an integer in [1, tracklog = {}]".format(fn, self.log_L))
        m = self.motion_scalars
        scal = dict(q=m["q"] if q is None else float(q), r=m["r"] if r is None else float(r), v0=m["v0_var"] if v0 is None else float(v0))
        for name, v in scal.items():
            if not 0.0 < v < float("inf"):   # (NaN fails too)
                raise ValueError("SqairStream.{}: {} must be finite and > 0".format(fn, name))
        return lag, scal

    def _solve_log(self, lag, scal):
        """The solve's launch on the current stream (include/sqair_hip.h: sqair_lane_tracklog_smooth) into the outputs and scratch of
        ``lag`` -- kept for the LAST lag asked for, with what the scorer and the fit add to them; returns them."""
        core, B, Cn = self.core, self.B, self.log_C
        if self._log_out.get("lag") != lag:
            out = zeros_of("SqairTrackLogOut", _capi.tracklog_out_shapes(lag, B, Cn), core.device)
            nbytes = B * core.lib.sqair_lane_tracklog_work_bytes(lag, Cn, core.N)
            self._log_out = dict(lag=lag, out=out, work=torch.zeros(nbytes // 4, dtype=torch.int32, device=core.device),
                                 c=_capi.SqairTrackLogOut(**{n: t.data_ptr() for n, t in out.items()}))
            torch.cuda.current_stream(core.device).synchronize()
        o = self._log_out
        core.check(core.lib.sqair_lane_tracklog_smooth(core.handle, C.byref(self._log_c), lag, Cn, core.N, B, scal["q"],
                                                       scal["r"], scal["v0"], C.byref(o["c"]), o["work"].data_ptr(),
                                                       core._stream()), "sqair_lane_tracklog_smooth")
        return o

    def track_log(self, lag=None, q=None, r=None, v0=None, score=False, score_iou=0.5, score_match="greedy", stitch=False,
                  stitch_gate=3.5, stitch_max_gap=None):
        lag, scal = self._check_log_call("track_log", lag, q, r, v0)
        if score:
            if not self.log_G:
                raise ValueError("SqairStream.track_log: score=True is for a stream that keeps the log's truth (SqairStream(..., "
                                 "tracklog=L, tracklog_truth=G))")
            score_iou = float(score_iou)
            check_unit("SqairStream.track_log: ", "score_iou", score_iou)
            if score_match not in MATCH_MODES:
                raise ValueError("SqairStream.track_log: score_match must be 'greedy' or 'optimal'")
        if stitch:
            try:
                stitch_gate = float(stitch_gate)
            except (TypeError, ValueError):
                stitch_gate = float("nan")
            if not 0.0 < stitch_gate < float("inf"):   # (NaN fails too)
                raise ValueError("SqairStream.track_log: stitch_gate must be finite and > 0")
            stitch_max_gap = lag if stitch_max_gap is None else stitch_max_gap
            if not is_int_in(stitch_max_gap, 0, lag):
                raise ValueError("SqairStream.track_log: stitch_max_gap must be an integer in [0, lag = {}]".format(lag))
        core = self.core
        match = MATCH_MODES.index(score_match) if score else 0
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                o = self._solve_log(lag, scal)
                got = {n: t.clone() for n, t in o["out"].items()}
                scored = self._score_log(o, o["out"], "score", lag, score_iou, match) if score else None
                if stitch:
                    st = self._stitch_log(o, lag, scal, stitch_gate, int(stitch_max_gap))
                    joined = {n: t.clone() for n, t in st["out"].items()}
                    links = {n: t.clone() for n, t in st["links"].items()}
                    joined_score = self._score_log(o, st["out"], "stitch_score", lag, score_iou, match) if score else None
            core._join_out()
        res = track_log_views({n: t.cpu() for n, t in got.items()})
        if scored is not None:
            res["score"] = track_log_score({n: t.cpu() for n, t in scored.items()})
        if stitch:
            res["stitched"] = track_log_views({n: t.cpu() for n, t in joined.items()})
            res["stitched"]["links"] = {name: links[field].cpu() for name, field in _capi.TRACKLOG_STITCH_LINKS.items()}
            if joined_score is not None:
                res["stitched"]["score"] = track_log_score({n: t.cpu() for n, t in joined_score.items()})
        return res

    def _stitch_log(self, o, lag, scal, gate, max_gap):
        """The stitch directly behind the solve, on the current stream and on the solve's device tensors ``o`` (include/sqair_hip.h:
        sqair_lane_tracklog_stitch): one launch into a second table, a second ``work`` and the link outputs, kept with the solve's."""
        core, B, Cn = self.core, self.B, self.log_C
        if "stitch" not in o:   # (the outputs belong to the solve's lag: another lag has dropped them with the rest)
            out = zeros_of("SqairTrackLogOut", _capi.tracklog_out_shapes(lag, B, Cn), core.device)
            o["stitch"] = dict(out=out, work=torch.zeros_like(o["work"]),
                               links=zeros_of("SqairTrackLogStitch", _capi.tracklog_stitch_shapes(B, Cn), core.device),
                               c=_capi.SqairTrackLogOut(**{n: t.data_ptr() for n, t in out.items()}))
            torch.cuda.current_stream(core.device).synchronize()
        st = o["stitch"]
        c_st = _capi.SqairTrackLogStitch(gate=gate, max_gap=max_gap, **{n: t.data_ptr() for n, t in st["links"].items()})
        core.check(core.lib.sqair_lane_tracklog_stitch(core.handle, C.byref(self._log_c), C.byref(o["c"]), o["work"].data_ptr(), lag, Cn,
                                                       core.N, B, scal["q"], scal["r"], scal["v0"], C.byref(c_st), C.byref(st["c"]),
                                                       st["work"].data_ptr(), core._stream()), "sqair_lane_tracklog_stitch")
        return st

    def _score_log(self, o, table, key, lag, iou_min, match):
        """The scorer on the current stream and on the device tensors ``table`` -- the solve's ``o["out"]``, directly behind it, or the
        stitch's, behind that (include/sqair_hip.h: sqair_lane_tracklog_score) --, its outputs kept under ``o[key]``: the truth ring
        gathered into window order -- window frame f of every lane is stream frame ring_frames - lag + f; a frame before the ring
        existed is invalid --, one launch, the outputs' copies."""
        core, B, G, n = self.core, self.B, self.log_G, self.ring_frames
        if key not in o:   # (the outputs belong to the solve's lag: another lag has dropped them with the rest)
            o[key] = zeros_of("SqairTrackLogScore", _capi.tracklog_score_shapes(lag, B, G), core.device)
        truth = {k: ring_window(t, n, lag) for k, t in self.truth_ring.items()}
        if n < lag:
            truth["truth_valid"][:lag - n].zero_()
        c_tab = _capi.SqairTrackLogOut(**{k: table[k].data_ptr() for k in _capi.TRACKLOG_SCORE_TABLE})
        c_truth = _capi.SqairTrackLogTruth(G=G, **{k: t.data_ptr() for k, t in truth.items()})
        c_score = _capi.SqairTrackLogScore(iou_min=iou_min, **{k: t.data_ptr() for k, t in o[key].items()})
        core.check(core.lib.sqair_lane_tracklog_score(core.handle, C.byref(self._log_c), C.byref(c_tab), C.byref(c_truth), C.byref(c_score),
                                                      lag, self.log_C, B, match, core._stream()), "sqair_lane_tracklog_score")
        return {k: t.clone() for k, t in o[key].items()}

    def _check_grid(self, name, grid, centre):
        """A grid of ``track_log_fit`` as a list of floats (None: ``centre`` * 4^k, k = -4..3, so that ``centre`` is node 4)."""
        if grid is None:
            grid = [centre * 4.0 ** k for k in range(-4, 4)]
        try:
            grid = [float(v) for v in (grid.tolist() if hasattr(grid, "tolist") else grid)]
        except (TypeError, ValueError):
            grid = []
        if not 1 <= len(grid) <= _capi.TRACKLOG_FIT_MAX_GRID:
            raise ValueError("SqairStream.track_log_fit: {} must hold 1 to {} values".format(name, _capi.TRACKLOG_FIT_MAX_GRID))
        if not all(0.0 < v < float("inf") for v in grid):   # (NaN fails too)
            raise ValueError("SqairStream.track_log_fit: every value of {} must be finite and > 0".format(name))
        return grid

    def track_log_fit(self, lag=None, q_grid=None, r_grid=None, v0=None, burn=2, innov=False):
        lag, scal = self._check_log_call("track_log_fit", lag, None, None, v0)
        q_grid = self._check_grid("q_grid", q_grid, scal["q"])
        r_grid = self._check_grid("r_grid", r_grid, scal["r"])
        if not is_int_in(burn, 0, 2 ** 31 - 1):
            raise ValueError("SqairStream.track_log_fit: burn must be an integer >= 0")
        core, B, Cn = self.core, self.B, self.log_C
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                o = self._solve_log(lag, scal)   # (state and the slots do not depend on q and r: the stream's own serve)
                key = (len(q_grid), len(r_grid))
                if o.get("fit_key") != key:   # (the outputs belong to the solve's lag and to the grid's size)
                    o["fit"] = zeros_of("SqairTrackLogFit", _capi.tracklog_fit_shapes(lag, B, Cn, *key), core.device)
                    o["fit_key"] = key
                    torch.cuda.current_stream(core.device).synchronize()
                buf = {k: t for k, t in o["fit"].items() if innov or k in _capi.TRACKLOG_FIT_REQUIRED}
                c_tab = _capi.SqairTrackLogOut(**{k: o["out"][k].data_ptr() for k in _capi.TRACKLOG_FIT_TABLE})
                c_fit = _capi.tracklog_fit_struct(q_grid, r_grid, scal["v0"], int(burn), **{k: t.data_ptr() for k, t in buf.items()})
                core.check(core.lib.sqair_lane_tracklog_fit(core.handle, C.byref(self._log_c), C.byref(c_tab), o["work"].data_ptr(),
                                                            C.byref(c_fit), lag, Cn, core.N, B, core._stream()), "sqair_lane_tracklog_fit")
                got = {k: t.clone() for k, t in buf.items()}
            core._join_out()
        return track_log_fit({k: t.cpu() for k, t in got.items()}, q_grid, r_grid)

    def set_motion(self, q=None, r=None, v0=None, gate=None):
        """``SqairStream.set_motion``'s part here: the scalars checked and kept; on a stream with ``motion=True`` the motion registered
        again with them and the same buffers.  Returns whether the pass changed (a captured graph is then stale)."""
        new = dict(self.motion_scalars)
        for key, name, v in (("q", "q", q), ("r", "r", r), ("v0_var", "v0", v0), ("gate", "gate", gate)):
            if v is None:
                continue
            try:
                new[key] = float(v)
            except (TypeError, ValueError):
                new[key] = float("nan")
            if not 0.0 < new[key] < float("inf"):   # (NaN fails too)
                raise ValueError("SqairStream.set_motion: {} must be finite and > 0".format(name))
        self.motion_scalars = new
        if not self.motion:
            return False
        core, est = self.core, self.est
        mo = _capi.SqairLaneMotion(trk_kf=self.ident_buf["trk_kf"].data_ptr(), **new,
                                   **{n: est[n].data_ptr() for n in _capi.MOTION_FIELDS if n in est})
        core.stream.synchronize()   # (no pass in flight reads the scalars being replaced)
        core.check(core.lib.sqair_set_motion(core.handle, C.byref(mo), self.T, self.B), "sqair_set_motion")
        return True

    def identities(self):
        if not self.identified:
            raise ValueError("SqairStream.identities: the stream keeps no identities (SqairStream(..., estimate=True, identity=True))")
        names = ("counts", "next_id", "trk_id", "trk_age", "trk_len", "trk_box") + (_capi.MOTION_MEMORY if self.motion else ())
        got = read_back(self.core, {n: self.ident_buf[n] for n in names})
        res = _columns(got.pop("counts"), _capi.IDENT_COUNTS)
        tot = {n: int(v.sum()) for n, v in res.items()}
        res.update(got)
        if self.motion:   # the filter's state by name; the coasted box is formed here, on the host, from the table read back
            kf = _columns(res.pop("trk_kf"), _capi.MOTION_STATE)
            res["trk_centre"], res["trk_vel"], res["trk_sigma"] = kf["p"], kf["v"], kf["Ppp"].sqrt()
            size = res["trk_box"][..., 2:]
            res["trk_pred_box"] = torch.cat([kf["p"] - 0.5 * size, size], -1)
        res["bridged_rate"] = _ratio(tot["bridged"], tot["objects"])
        res["reidentified_rate"] = _ratio(tot["reidentified"], tot["objects"])
        return res


# ---- the per-call trajectory scores of forecast() and tracks() -------------------------------------------------------------------
class TrajScores(object):
    """``acc``: by kind ("forecast", "tracks") the accumulators and per-call outputs of the LAST (F, G, truth_iou, link_match) scored.  ``lane``:
    the stream's LaneAnswers (``link_ids`` keeps a truth with the identity its score last matched it with)."""

    def __init__(self, core, B, lane):
        self.core, self.B, self.lane, self.acc = core, B, lane, {}

    def check_truth(self, fn, truth, lane, F, default_anchor, link_ids, truth_iou, link_match="greedy"):
        """``truth`` of ``forecast`` / ``tracks`` as {name: tensor} in the C ABI's names and dtypes plus ``G`` and ``iou_min`` (None: no
        truth); everything is checked here, ``link_match`` too, before the core is touched."""
        if link_match not in MATCH_MODES:
            raise ValueError(fn + "link_match must be 'greedy' or 'optimal'")
        if truth is None:
            if link_ids:
                raise ValueError(fn + "link_ids is for a call with truth")
            if link_match == "optimal":
                raise ValueError(fn + "link_match='optimal' is for a call with truth")
            return None
        if not lane:
            raise ValueError(fn + "truth is for a call with lane=True: the lane table is what is scored")
        names = {"box", "present", "valid", "anchor_box", "anchor_present", "anchor_valid"}
        if not isinstance(truth, dict) or "box" not in truth or "present" not in truth or set(truth) - names:
            raise ValueError(fn + "truth must be a dict with box, present and optionally valid, anchor_box, anchor_present, anchor_valid")
        truth_iou = float(truth_iou)
        check_unit(fn, "truth_iou", truth_iou)
        B = self.B
        box = torch.as_tensor(truth["box"]).to(torch.float32)
        present = torch.as_tensor(truth["present"])
        if box.dim() != 4 or not 1 <= box.shape[2] <= _capi.SCORE_MAX_TRUTH:
            raise ValueError(fn + "truth['box'] of shape {} given, [{}, {}, G, 4] with G in [1, {}] expected".format(
                tuple(box.shape), F, B, _capi.SCORE_MAX_TRUTH))
        G = int(box.shape[2])
        given = truth.get("valid") is not None
        valid = torch.as_tensor(truth["valid"]) if given else torch.ones((F, B), dtype=torch.int32)
        check_shapes(fn, (("box", box, (F, B, G, 4)), ("present", present, (F, B, G)), ("valid", valid, (F, B))))
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
        check_shapes(fn, (("anchor_box", a_box, (B, G, 4)), ("anchor_present", a_present, (B, G)), ("anchor_valid", a_valid, (B,))))
        if link_ids and not (self.lane.scored and G == self.lane.G):
            raise ValueError(fn + "link_ids is for a stream with score=True and the same G: it keeps a truth with the identity the "
                                  "stream's score last matched it with")
        return dict(G=G, iou_min=truth_iou, truth_box=box, truth_present=as_mask(present), truth_valid=as_mask(valid), anchor_box=a_box,
                    anchor_present=as_mask(a_present), anchor_valid=as_mask(a_valid))

    def launch(self, kind, table, F, truth, link_ids, link_match="greedy"):
        """Scores the lane table a forecast or a trace has just written (``table``: its device buffers by field) against ``truth``
        (of check_truth) with one launch on the core's stream (include/sqair_hip.h: sqair_lane_traj_score); returns the per-call
        outputs, copies.  The accumulators of ``kind`` are kept for the last (F, G, truth_iou, link_match) scored."""
        core, B = self.core, self.B
        match = MATCH_MODES.index(link_match)
        G, key = truth["G"], (F, truth["G"], truth["iou_min"], match)
        ts = self.acc.get(kind)
        if ts is None or ts["key"] != key:   # (another F, G, threshold or matching: the old sums would not mean the same)
            ts = self.acc[kind] = dict(zeros_of("SqairTrajScore", dict(counts=(F, B, len(_capi.TRAJ_COUNTS)), sums=(F, B, len(_capi.TRAJ_SUMS)),
                                                                       lane_counts=(B, len(_capi.TRAJ_LANE_COUNTS))), core.device), key=key)
            ts["flat"], ts["views"] = field_views(_capi.traj_shapes(F, B, G), _capi.TRAJ_INT_FIELDS, core.device)
            ts["out"] = ts["views"](ts["flat"])
        dev = {n: truth[n].to(core.device, non_blocking=True).contiguous() for n in _capi.TRAJ_TRUTH_FIELDS if n != "keep_id"}
        c_tab = _capi.SqairLaneTraj(**{n: table[n].data_ptr() for n in _capi.TRAJ_TABLE_FIELDS if n in table})
        c_truth = _capi.SqairTrajTruth(G=G, keep_id=self.lane.score_buf["last_id"].data_ptr() if link_ids else None,
                                       **{n: t.data_ptr() for n, t in dev.items()})
        c_score = _capi.SqairTrajScore(iou_min=truth["iou_min"], **{n: ts[n].data_ptr() for n in _capi.TRAJ_ACCUMULATORS},
                                       **{n: t.data_ptr() for n, t in ts["out"].items()})
        # (the link's mode is the call's; the score's and the identity's stay the stream's: the handle holds all three)
        core.check(core.lib.sqair_set_lane_match(core.handle, self.lane.score_match, self.lane.identity_match, match),
                   "sqair_set_lane_match")
        core.check(core.lib.sqair_lane_traj_score(core.handle, C.byref(c_tab), C.byref(c_truth), C.byref(c_score), F, B,
                                                  core._stream()), "sqair_lane_traj_score")
        return ts["views"](ts["flat"].clone())

    def read(self, kind, reset=False):
        if kind not in ("forecast", "tracks"):
            raise ValueError("SqairStream.trajectory_score: kind must be 'forecast' or 'tracks'")
        ts = self.acc.get(kind)
        if ts is None:
            raise ValueError("SqairStream.trajectory_score: no {} call has been scored yet ({}(..., lane=True, truth=...))".format(kind, kind))
        acc = read_back(self.core, {n: ts[n] for n in _capi.TRAJ_ACCUMULATORS}, zero=reset)
        res = _columns(acc["counts"], _capi.TRAJ_COUNTS)
        res.update(_columns(acc["sums"], _capi.TRAJ_SUMS))
        res.update(_columns(acc["lane_counts"], _capi.TRAJ_LANE_COUNTS))
        tot = {n: res[n].sum(1).to(torch.float64) for n in _capi.TRAJ_COUNTS + _capi.TRAJ_SUMS}
        div = lambda a, b: torch.where(b > 0, a / torch.where(b > 0, b, torch.ones_like(b)), torch.full_like(b, float("nan")))
        res["ade"] = div(tot["centre_err_sum"], tot["pairs"])
        res["fde"] = float(res["ade"][-1])
        res["mean_iou"] = div(tot["iou_sum"], tot["pairs"])
        res["hit_rate"] = div(tot["hits"], tot["pairs"] + tot["lost"])
        res["brier"] = div(tot["brier_sum"], tot["pairs"] + tot["lost"] + tot["gone"])
        res["count_accuracy"] = div(tot["count_hit"], tot["frames"])
        res["link_rate"] = _ratio(int(res["linked"].sum()), int(res["anchor_truth"].sum()))
        return res
