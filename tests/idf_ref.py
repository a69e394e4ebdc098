"""The integer / float64 reference of IDF1 scoring (include/sqair_hip.h: sqair_set_idf, points 1-5), restated from the header and not
from the kernels: NumPy, plain loops over (lane, frame).  Only the boxes are fp32 words; the IoU computed from them is float64
(tests/score_ref.py: iou_table); everything after the threshold is integer.  The assignment is solved two ways: SciPy's
linear_sum_assignment, and brute force over the permutations for small tables.  ``fragile_from`` is the rule by which a lane is left
out of an exact comparison from its first frame on which a present pair's IoU lies within the measured fp32 error of iou_min."""
import itertools

import numpy as np

from tests import score_ref as SR

TOTALS = ("clips", "frames", "trajectories", "idtp", "idfn", "idfp", "mt", "pt", "ml", "frag", "ids", "overflow_ids")
TABLE = ("col_id", "overlap", "row_frames", "col_frames", "extra_frames", "matched", "frag", "trk_state", "frames")


def new_table(B, G, P):
    """A fresh table {name: int32 array} and ``totals`` [B, 12] int64: col_id -1, everything else 0."""
    t = dict(col_id=-np.ones((B, P), np.int32), overlap=np.zeros((B, G, P), np.int32), row_frames=np.zeros((B, G), np.int32),
             col_frames=np.zeros((B, P), np.int32), extra_frames=np.zeros(B, np.int32), matched=np.zeros((B, G), np.int32),
             frag=np.zeros((B, G), np.int32), trk_state=np.zeros((B, G), np.int32), frames=np.zeros(B, np.int32),
             totals=np.zeros((B, len(TOTALS)), np.int64))
    return t


def copy_table(t):
    return {n: np.array(v) for n, v in t.items()}


def accumulate(table, box, presence, ids, map_count, truth_box, truth_present, truth_valid, truth_match, iou_min):
    """Point 3 for passes of T frames, continuing ``table`` (a new one is returned): box [T, B, N, 4], presence [T, B, N], ids
    [T, B, N] int32 words, map_count [T, B]; truth_box [T, B, G, 4], truth_present, truth_match [T, B, G], truth_valid [T, B]."""
    t = copy_table(table)
    T, B, G = np.asarray(truth_present).shape
    N = np.asarray(presence).shape[2]
    P = t["col_id"].shape[1]
    iou_min = float(np.float32(iou_min))
    iou = SR.iou_table(truth_box, box)
    for b in range(B):
        for f in range(T):
            if truth_valid[f, b] == 0 or map_count[f, b] == -1:
                continue
            t["frames"][b] += 1
            col = -np.ones(N, np.int64)
            unkeyed = 0
            for j in range(N):
                if presence[f, b, j] == 0:
                    continue
                word = int(ids[f, b, j])
                c = -1
                if word >= 0:
                    hit = np.flatnonzero(t["col_id"][b] == word)
                    free = np.flatnonzero(t["col_id"][b] < 0)
                    if hit.size:
                        c = int(hit[0]) if int(hit[0]) not in col[:j] else -1
                    elif free.size:
                        c = int(free[0])
                        t["col_id"][b, c], t["col_frames"][b, c], t["overlap"][b, :, c] = word, 0, 0
                if c < 0:
                    unkeyed += 1
                    continue
                col[j] = c
                t["col_frames"][b, c] += 1
            t["extra_frames"][b] += unkeyed
            t["totals"][b, TOTALS.index("overflow_ids")] += unkeyed > 0
            for g in range(G):
                if truth_present[f, b, g] == 0:
                    continue
                t["row_frames"][b, g] += 1
                for j in range(N):
                    if col[j] >= 0 and iou[f, b, g, j] >= iou_min:
                        t["overlap"][b, g, col[j]] += 1
                m = int(truth_match[f, b, g] >= 0)
                st = int(t["trk_state"][b, g])
                t["matched"][b, g] += m
                t["frag"][b, g] += int(m and (st & 2) and not (st & 1))
                t["trk_state"][b, g] = (st & 2) | (3 if m else 0)
    return t


def best_scipy(w):
    """The maximum over one-to-one assignments of rows to columns of the sum of w (unassigned allowed: negative weights are never
    taken); returns (optimum, row_to_col with -1 for a row left out or assigned at weight <= 0)."""
    from scipy.optimize import linear_sum_assignment
    w = np.maximum(np.asarray(w, np.int64), 0)
    r2c = -np.ones(w.shape[0], np.int64)
    if w.size == 0:
        return 0, r2c
    r, c = linear_sum_assignment(w, maximize=True)
    for i, j in zip(r, c):
        if w[i, j] > 0:
            r2c[i] = j
    return int(w[r, c].sum()), r2c


def best_brute(w):
    """The same optimum by brute force: every injection of the smaller side into the larger (small tables only)."""
    w = np.maximum(np.asarray(w, np.int64), 0)
    if w.shape[0] > w.shape[1]:
        w = w.T
    G, P = w.shape
    return max((int(sum(w[g, p] for g, p in enumerate(perm))) for perm in itertools.permutations(range(P), G)), default=0)


def masked_overlap(table, b):
    """Lane b's overlap table with the free columns as zeros (their words are never read)."""
    return np.where(table["col_id"][b][None, :] >= 0, table["overlap"][b], 0).astype(np.int64)


def figures(table, b, solver=best_scipy):
    """Point 4 for lane b: the clip's twelve figures (int64, TOTALS' order) and the optimal row_to_col."""
    w = masked_overlap(table, b)
    got = solver(w)
    idtp, r2c = got if isinstance(got, tuple) else (got, None)
    used = table["col_id"][b] >= 0
    rf, m = table["row_frames"][b].astype(np.int64), table["matched"][b].astype(np.int64)
    traj = rf > 0
    mt = traj & (5 * m >= 4 * rf)
    ml = traj & (5 * m < rf)
    frames = int(table["frames"][b])
    fig = np.array([int(frames > 0), frames, traj.sum(), idtp, rf.sum() - idtp,
                    table["col_frames"][b][used].sum() + int(table["extra_frames"][b]) - idtp, mt.sum(), (traj & ~mt & ~ml).sum(), ml.sum(),
                    table["frag"][b].sum(), used.sum(), 0], np.int64)
    return fig, r2c


def solve(table, close=None, solver=best_scipy):
    """Points 4 and 5 for every lane: returns (table after, open [B, 12] int64).  ``close`` [B]: those lanes' figures go into totals
    and their tables are freed -- overlap and col_frames of a freed column stay as they are."""
    t = copy_table(table)
    B = t["col_id"].shape[0]
    open_ = np.zeros((B, len(TOTALS)), np.int64)
    for b in range(B):
        open_[b], _ = figures(t, b, solver)
        if close is not None and close[b] != 0:
            t["totals"][b] += open_[b]
            t["col_id"][b] = -1
            for n in ("row_frames", "matched", "frag", "trk_state"):
                t[n][b] = 0
            t["extra_frames"][b] = t["frames"][b] = 0
    return t, open_


def pooled(per_lane):
    """idf1, idp, idr, mt_rate, ml_rate, frag and exact over the lanes of ``per_lane`` [B, 12]; NaN where a denominator is 0."""
    c = dict(zip(TOTALS, np.asarray(per_lane).sum(0).tolist()))
    div = lambda a, b: float(a) / b if b else float("nan")
    return dict(idf1=div(2 * c["idtp"], 2 * c["idtp"] + c["idfp"] + c["idfn"]), idp=div(c["idtp"], c["idtp"] + c["idfp"]),
                idr=div(c["idtp"], c["idtp"] + c["idfn"]), mt_rate=div(c["mt"], c["trajectories"]), ml_rate=div(c["ml"], c["trajectories"]),
                frag=c["frag"], exact=c["overflow_ids"] == 0)


def check_assign(table, b, assign, idtp):
    """``assign`` [G] (id words, -1 none) of lane b is one-to-one over the used columns and its weight sums to ``idtp``."""
    words = [int(a) for a in assign if a >= 0]
    assert len(set(words)) == len(words), (b, assign)
    cid = table["col_id"][b].tolist()
    total = 0
    for g, a in enumerate(assign):
        if a >= 0:
            assert int(a) in cid, (b, g, a)
            total += int(table["overlap"][b, g, cid.index(int(a))])
    assert total == idtp, (b, total, idtp)


def fragile_from(iou, presence, map_count, truth_present, truth_valid, iou_min, near):
    """[B]: the first frame of each lane on which some present (truth, lane object) pair's float64 IoU lies within ``near`` of
    iou_min (T where none does): from there on the device's fp32 IoU may fall on the other side and the tables differ."""
    T, B, G, N = iou.shape
    iou_min = float(np.float32(iou_min))
    scored = (np.asarray(truth_valid) != 0) & (np.asarray(map_count) != -1)
    cand = (np.asarray(truth_present) != 0)[:, :, :, None] & (np.asarray(presence) != 0)[:, :, None, :] & scored[:, :, None, None]
    bad = (cand & (np.abs(iou - iou_min) <= near)).any((2, 3))   # [T, B]
    return np.where(bad.any(0), bad.argmax(0), T)
