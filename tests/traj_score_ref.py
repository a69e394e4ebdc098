"""The float64 reference of trajectory scoring (include/sqair_hip.h: sqair_lane_traj_score, points 0-6), restated from the header and
not from the kernel: NumPy.  Only the table's and the truth's words are fp32; everything computed from them is float64.  The link's
assignment is the score's (tests/score_ref.py: assign -- the header says it is the same device function, unchanged).
``frame_values`` computes the per-frame quantities in a chosen arithmetic: float64 for the reference, float32 for the restatement the
GPU test's bars are measured with (``fp32_errors``).  ``fragile_lanes`` is the rule by which a lane is left out of an exact
comparison: a decision of it hangs on less than the bar."""
import collections

import numpy as np

from tests.score_ref import assign, iou32, iou64, words

COUNTS = ("frames", "pairs", "hits", "lost", "gone", "count_hit", "count_abs_err")
SUMS = ("iou_sum", "centre_err_sum", "brier_sum")
LANE_COUNTS = ("calls", "calls_invalid", "anchor_truth", "linked")
INT_OUT = ("link", "state", "count_map")
FLOAT_OUT = ("link_iou", "p_alive", "pair_iou", "centre_err")
BAR_FACTOR = 4.0        # the GPU bars are this many times the fp32 restatement's measured error (as the score's test)

Traj = collections.namedtuple("Traj", "link link_iou state p_alive pair_iou centre_err count_map brier counts sums lane_counts iou")
_IOU = {np.float64: iou64, np.float32: iou32}


def anchor_iou(tab, tr, ft=np.float64):
    """[B, G, N]: IoU of every anchor truth with every lane object, present or not."""
    return _IOU[ft](np.asarray(tr["anchor_box"], np.float32)[:, :, None, :], np.asarray(tab["box0"], np.float32)[:, None, :, :])


def frame_values(tab, tr, link, ft):
    """p_alive, pair_iou, centre_err, brier [F, B, G] in the arithmetic of ``ft`` for truth g against lane object link[b, g], for every
    (f, b, g) whether it is scored or not (the caller masks; an unlinked g reads object 0 and means nothing)."""
    B, G = link.shape
    j, bi = np.maximum(link, 0), np.arange(B)[:, None]
    with np.errstate(all="ignore"):
        alive = np.asarray(tab["alive"], np.float32)[:, bi, j].astype(ft)
        support = np.asarray(tab["support"], np.float32)[bi, j].astype(ft)
        p = alive / support[None]
        y = (np.asarray(tr["truth_present"]) != 0).astype(ft)
        d = p - y
        brier = d * d
        q = np.asarray(tab["box_mean"], np.float32)[:, bi, j]
        tb = np.asarray(tr["truth_box"], np.float32)
        iou = _IOU[ft](tb, q)
        q, tb, half = q.astype(ft), tb.astype(ft), ft(0.5)
        dy = (tb[..., 0] + half * tb[..., 2]) - (q[..., 0] + half * q[..., 2])
        dx = (tb[..., 1] + half * tb[..., 3]) - (q[..., 1] + half * q[..., 3])
        err = np.sqrt(dy * dy + dx * dx)
    return p.astype(ft), iou.astype(ft), err.astype(ft), brier.astype(ft)


def lane_on(tab, tr):
    """[B]: lanes that are scored -- a valid anchor and a finite lane."""
    return (np.asarray(tr["anchor_valid"]) != 0) & (np.asarray(tab["best_row"]) != -1)


def frames_on(tab, tr):
    """[F, B]: (frame, lane)s that are scored."""
    on = lane_on(tab, tr)[None] & (np.asarray(tr["truth_valid"]) != 0)
    if tab.get("valid_mass") is not None:
        with np.errstate(invalid="ignore"):
            on = on & (np.asarray(tab["valid_mass"]) > 0)
    return on


def link_lanes(tab, tr, iou_min, keep_id=None):
    """Point 1: link [B, G] (j or -1) and the anchor IoU table [B, G, N] in float64."""
    B, G = np.asarray(tr["anchor_present"]).shape
    iou = anchor_iou(tab, tr)
    on = lane_on(tab, tr)
    ids = words(tab["obj_id"]) if tab.get("obj_id") is not None else np.zeros(np.asarray(tab["presence"]).shape, np.int32)
    link = -np.ones((B, G), np.int64)
    none = -np.ones(G, np.int64)
    for b in np.nonzero(on)[0]:
        link[b], _ = assign(iou[b], np.asarray(tr["anchor_present"][b]) != 0, np.asarray(tab["presence"][b]) != 0, ids[b],
                            none if keep_id is None else np.asarray(keep_id[b]), iou_min)
    return link, iou


def score(tab, tr, iou_min, keep_id=None, counts=None, sums=None, lane_counts=None):
    """The header's points for one call.  ``tab``: best_row [B], presence, obj_id, support [B, N], box0 [B, N, 4], alive [F, B, N],
    box_mean [F, B, N, 4], count_prob [F, B, N + 1] and optionally valid_mass [F, B]; ``tr``: anchor_box [B, G, 4], anchor_present
    [B, G], anchor_valid [B], truth_box [F, B, G, 4], truth_present [F, B, G], truth_valid [F, B].  ``counts`` [F, B, 7], ``sums``
    [F, B, 3], ``lane_counts`` [B, 4]: what to continue from (default: zeros); the returned ones are new arrays."""
    F, B, G = np.asarray(tr["truth_present"]).shape
    iou_min = float(np.float32(iou_min))
    counts = np.zeros((F, B, len(COUNTS)), np.int64) if counts is None else np.array(counts, np.int64)
    sums = np.zeros((F, B, len(SUMS)), np.float64) if sums is None else np.array(sums, np.float64)
    lane_counts = np.zeros((B, len(LANE_COUNTS)), np.int64) if lane_counts is None else np.array(lane_counts, np.int64)
    on_lane, on = lane_on(tab, tr), frames_on(tab, tr)
    # 1: the link
    link, iou = link_lanes(tab, tr, iou_min, keep_id)
    linked = link >= 0
    link_iou = np.where(linked, np.take_along_axis(iou, np.maximum(link, 0)[:, :, None], 2)[:, :, 0], 0.0)
    anchored = np.asarray(tr["anchor_valid"]) != 0
    apres = (np.asarray(tr["anchor_present"]) != 0) & on_lane[:, None]
    lane_counts[:, 0] += on_lane
    lane_counts[:, 1] += anchored & ~on_lane
    lane_counts[:, 2] += apres.sum(1)
    lane_counts[:, 3] += linked.sum(1)
    # 2: the frames
    p, pair, err, brier = frame_values(tab, tr, link, np.float64)
    y = np.asarray(tr["truth_present"]) != 0
    sel = on[:, :, None] & linked[None]
    bi = np.arange(B)[:, None]
    with np.errstate(invalid="ignore"):
        living = np.asarray(tab["alive"], np.float32)[:, bi, np.maximum(link, 0)] > 0
    state = np.where(sel, np.where(~y, 0, np.where(living, 1, 2)), -1).astype(np.int32)
    is_pair = state == 1
    p_alive, brier = np.where(sel, p, 0.0), np.where(sel, brier, 0.0)
    pair_iou, centre_err = np.where(is_pair, pair, 0.0), np.where(is_pair, err, 0.0)
    # 3: the count
    count_map = np.where(on, np.argmax(np.asarray(tab["count_prob"], np.float32), -1), -1).astype(np.int32)
    n_truth = y.sum(-1)
    # 4: the accumulators
    add = (on, is_pair.sum(-1), (is_pair & (pair_iou >= iou_min)).sum(-1), (state == 2).sum(-1), (state == 0).sum(-1),
           on & (count_map == n_truth), np.where(on, np.abs(count_map - n_truth), 0))
    for i, v in enumerate(add):
        counts[:, :, i] += v
    for i, v in enumerate((pair_iou, centre_err, brier)):
        for g in range(G):
            sums[:, :, i] += v[:, :, g]
    return Traj(link.astype(np.int32), link_iou, state, p_alive, pair_iou, centre_err, count_map, brier, counts, sums, lane_counts, iou)


def fp32_errors(tab, tr, ref):
    """The worst |fp32 restatement - float64| of link_iou, p_alive, pair_iou, centre_err and the Brier term over the entries the
    reference uses, with the reference's link: what the GPU test's bars are BAR_FACTOR times of."""
    link = ref.link.astype(np.int64)
    p, pair, err, brier = frame_values(tab, tr, link, np.float32)
    sel, is_pair = ref.state >= 0, ref.state == 1
    worst = lambda a, want, m: float(np.abs(a.astype(np.float64) - want)[m].max()) if m.any() else 0.0
    cand = ((np.asarray(tr["anchor_present"]) != 0)[:, :, None] & (np.asarray(tab["presence"]) != 0)[:, None, :] &
            lane_on(tab, tr)[:, None, None])
    return dict(link_iou=worst(anchor_iou(tab, tr, np.float32), ref.iou, cand), p_alive=worst(p, ref.p_alive, sel),
                pair_iou=worst(pair, ref.pair_iou, is_pair), centre_err=worst(err, ref.centre_err, is_pair),
                brier=worst(brier, ref.brier, sel))


def bars(errors):
    return {n: BAR_FACTOR * e for n, e in errors.items()}


def fragile_lanes(tab, tr, ref, iou_min, bar):
    """[B] bool: lanes with a decision that hangs on less than ``bar`` -- a candidate of the link or a pair's IoU within ``bar`` of
    iou_min, or two candidates of the link that share a truth or a lane object, both within ``bar`` of passing, within ``bar`` of
    each other and not both exactly 1."""
    B, G, N = ref.iou.shape
    iou_min = float(np.float32(iou_min))
    out = np.zeros(B, bool)
    on = lane_on(tab, tr)
    near_pair = ((ref.state == 1) & (np.abs(ref.pair_iou - iou_min) <= bar)).any((0, 2))
    for b in np.nonzero(on)[0]:
        cand = (np.asarray(tr["anchor_present"][b]) != 0)[:, None] & (np.asarray(tab["presence"][b]) != 0)[None, :]
        v = ref.iou[b]
        bad = bool((cand & (np.abs(v - iou_min) <= bar)).any()) or bool(near_pair[b])
        pairs = np.argwhere(cand & (v >= iou_min - bar))
        for a in range(len(pairs)):
            for c in range(a + 1, len(pairs)):
                (g1, j1), (g2, j2) = pairs[a], pairs[c]
                if (g1 == g2 or j1 == j2) and abs(v[g1, j1] - v[g2, j2]) <= bar and not (v[g1, j1] == 1.0 and v[g2, j2] == 1.0):
                    bad = True
        out[b] = bad
    return out


def pooled(counts, sums, lane_counts):
    """The per-horizon curves pooled over the lanes, NaN where the denominator is 0, and link_rate."""
    c = {n: np.asarray(counts)[:, :, i].sum(1).astype(np.float64) for i, n in enumerate(COUNTS)}
    s = {n: np.asarray(sums)[:, :, i].sum(1) for i, n in enumerate(SUMS)}
    with np.errstate(all="ignore"):
        div = lambda a, b: np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)
        out = dict(ade=div(s["centre_err_sum"], c["pairs"]), mean_iou=div(s["iou_sum"], c["pairs"]),
                   hit_rate=div(c["hits"], c["pairs"] + c["lost"]), brier=div(s["brier_sum"], c["pairs"] + c["lost"] + c["gone"]),
                   count_accuracy=div(c["count_hit"], c["frames"]))
    out["fde"] = float(out["ade"][-1])
    lc = np.asarray(lane_counts).sum(0)
    out["link_rate"] = float(lc[3]) / lc[2] if lc[2] else float("nan")
    return out
