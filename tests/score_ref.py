"""The float64 reference of stream scoring (include/sqair_hip.h: sqair_set_score, points 0-6), restated from the header and not from
the kernel: NumPy, plain loops over (lane, frame).  Only the boxes are fp32 words; everything computed from them is float64.
``iou32`` is the fp32 restatement of sq_box_iou the tolerance of ``match_iou`` is measured with, ``fragile_from`` the rule by which a
lane is left out of an exact comparison from its first frame on which a decision hangs on less than 1e-5."""
import collections

import numpy as np

COUNTS = ("frames", "frames_invalid", "truth", "tp", "fn", "fp", "idsw", "count_hit", "count_abs_err")
NEAR = 1e-5

Score = collections.namedtuple("Score", "truth_match match_iou tp fn fp idsw counts iou_sum last_id iou")


def _iou(p, q, ft):
    """IoU of boxes p, q [..., 4] = (y, x, h, w) in the arithmetic of ``ft``; 0 when the union is not positive, exactly 1 for the
    same four words."""
    with np.errstate(invalid="ignore", over="ignore"):   # (a NaN word gives a NaN IoU, which no comparison accepts; NumPy warns, the device does not)
        same = (np.asarray(p) == np.asarray(q)).all(-1)
        p, q = np.asarray(p, ft), np.asarray(q, ft)
        zero = ft(0)
        oy = np.maximum(np.minimum(p[..., 0] + p[..., 2], q[..., 0] + q[..., 2]) - np.maximum(p[..., 0], q[..., 0]), zero)
        ox = np.maximum(np.minimum(p[..., 1] + p[..., 3], q[..., 1] + q[..., 3]) - np.maximum(p[..., 1], q[..., 1]), zero)
        inter = oy * ox
        uni = p[..., 2] * p[..., 3] + q[..., 2] * q[..., 3] - inter
        pos = uni > zero
        out = np.where(pos, inter / np.where(pos, uni, ft(1)), zero)
    return np.where(pos & same, ft(1), out).astype(ft)


def iou64(p, q):
    return _iou(p, q, np.float64)


def iou32(p, q):
    return _iou(p, q, np.float32)


def iou32_error(truth_box, box):
    """The worst |fp32 restatement - float64| of sq_box_iou over every (truth, lane object) pair of [T, B, G, 4] x [T, B, N, 4]."""
    a, b = np.asarray(truth_box, np.float32)[:, :, :, None, :], np.asarray(box, np.float32)[:, :, None, :, :]
    return float(np.abs(iou32(a, b).astype(np.float64) - iou64(a, b)).max())


def iou_table(truth_box, box):
    """[T, B, G, N] float64 IoU of every truth with every lane object, present or not."""
    return iou64(np.asarray(truth_box, np.float32)[:, :, :, None, :], np.asarray(box, np.float32)[:, :, None, :, :])


def words(obj_id):
    """The obj_id words: the 32 bits of the floats read as int32."""
    return np.ascontiguousarray(np.asarray(obj_id, np.float32)).view(np.int32)


def assign(iou, tpres, lpres, ids, last, iou_min):
    """Points 2 and 3 for one (frame, lane): iou [G, N], tpres [G], lpres [N], ids [N] (int words), last [G] -> match [G] (j or -1)."""
    G, N = iou.shape
    match = -np.ones(G, np.int64)
    claimed = np.zeros(N, bool)
    ok = lambda g, j: bool(tpres[g] and lpres[j] and iou[g, j] >= iou_min)   # (a NaN fails)
    for g in range(G):   # keep
        if last[g] < 0:
            continue
        for j in range(N):
            if not claimed[j] and ids[j] == last[g] and ok(g, j):
                match[g], claimed[j] = j, True
                break
    while True:          # rest: greedy
        best, arg = -1.0, None
        for g in range(G):
            if match[g] >= 0:
                continue
            for j in range(N):
                if not claimed[j] and ok(g, j) and iou[g, j] > best:
                    best, arg = iou[g, j], (g, j)
        if arg is None:
            break
        match[arg[0]], claimed[arg[1]] = arg[1], True
    return match, claimed


def score(box, presence, obj_id, map_count, truth_box, truth_present, truth_valid, iou_min, counts=None, iou_sum=None, last_id=None):
    """The header's points for passes of T frames: box [T, B, N, 4], presence, obj_id [T, B, N], map_count [T, B]; truth_box
    [T, B, G, 4], truth_present [T, B, G], truth_valid [T, B].  ``counts`` [B, 9], ``iou_sum`` [B], ``last_id`` [B, G]: the state to
    continue from (default: a fresh one); the returned ones are new arrays."""
    T, B, G = np.asarray(truth_present).shape
    N = np.asarray(presence).shape[2]
    iou_min = float(np.float32(iou_min))
    iou = iou_table(truth_box, box)
    ids = words(obj_id)
    counts = np.zeros((B, len(COUNTS)), np.int64) if counts is None else np.array(counts, np.int64)
    iou_sum = np.zeros(B, np.float64) if iou_sum is None else np.array(iou_sum, np.float64)
    last_id = -np.ones((B, G), np.int32) if last_id is None else np.array(last_id, np.int32)
    truth_match = -np.ones((T, B, G), np.int32)
    match_iou = np.zeros((T, B, G), np.float64)
    ev = {n: -np.ones((T, B), np.int32) for n in ("tp", "fn", "fp", "idsw")}
    C = {n: i for i, n in enumerate(COUNTS)}
    for b in range(B):
        for t in range(T):
            if truth_valid[t, b] == 0:
                continue
            if map_count[t, b] == -1:
                counts[b, C["frames_invalid"]] += 1
                continue
            tpres, lpres = np.asarray(truth_present[t, b]) != 0, np.asarray(presence[t, b]) != 0
            match, claimed = assign(iou[t, b], tpres, lpres, ids[t, b], last_id[b], iou_min)
            tp = fn = sw = 0
            for g in range(G):
                if not tpres[g]:
                    continue
                j = match[g]
                if j < 0:
                    fn += 1
                    continue
                tp += 1
                sw += int(last_id[b, g] >= 0 and last_id[b, g] != ids[t, b, j])
                last_id[b, g] = ids[t, b, j]
                truth_match[t, b, g] = j
                match_iou[t, b, g] = iou[t, b, g, j]
                iou_sum[b] += iou[t, b, g, j]
            fp = int((lpres & ~claimed).sum())
            n_truth = int(tpres.sum())
            ev["tp"][t, b], ev["fn"][t, b], ev["fp"][t, b], ev["idsw"][t, b] = tp, fn, fp, sw
            for n, v in (("frames", 1), ("truth", n_truth), ("tp", tp), ("fn", fn), ("fp", fp), ("idsw", sw),
                         ("count_hit", int(map_count[t, b] == n_truth)), ("count_abs_err", abs(int(map_count[t, b]) - n_truth))):
                counts[b, C[n]] += v
    return Score(truth_match, match_iou, ev["tp"], ev["fn"], ev["fp"], ev["idsw"], counts, iou_sum, last_id, iou)


def pooled(counts, iou_sum):
    """mota, motp and count_accuracy over the lanes of ``counts`` [B, 9]; NaN where a denominator is 0."""
    c = dict(zip(COUNTS, np.asarray(counts).sum(0).tolist()))
    div = lambda a, b: float(a) / b if b else float("nan")
    return dict(mota=1.0 - div(c["fn"] + c["fp"] + c["idsw"], c["truth"]), motp=div(float(np.sum(iou_sum)), c["tp"]),
                count_accuracy=div(c["count_hit"], c["frames"]))


def fragile_from(iou, presence, map_count, truth_present, truth_valid, iou_min):
    """[B]: the first fragile frame of each lane (T where none is).  A scored frame is fragile when a candidate IoU lies within 1e-5 of
    iou_min, or when two candidate pairs that share a truth or a lane object, both within 1e-5 of passing, lie within 1e-5 of each
    other and are not both exactly 1."""
    T, B, G, N = iou.shape
    iou_min = float(np.float32(iou_min))
    first = np.full(B, T, np.int64)
    for b in range(B):
        for t in range(T):
            if truth_valid[t, b] == 0 or map_count[t, b] == -1:
                continue
            cand = (np.asarray(truth_present[t, b]) != 0)[:, None] & (np.asarray(presence[t, b]) != 0)[None, :]
            v = iou[t, b]
            bad = bool((cand & (np.abs(v - iou_min) <= NEAR)).any())
            alive = cand & (v >= iou_min - NEAR)
            pairs = np.argwhere(alive)
            for a in range(len(pairs)):
                for c in range(a + 1, len(pairs)):
                    (g1, j1), (g2, j2) = pairs[a], pairs[c]
                    if (g1 == g2 or j1 == j2) and abs(v[g1, j1] - v[g2, j2]) <= NEAR and not (v[g1, j1] == 1.0 and v[g2, j2] == 1.0):
                        bad = True
            if bad:
                first[b] = t
                break
    return first
