"""The float64 reference of lane identities (include/sqair_hip.h: sqair_set_identity, points 0-9), restated from the header and not
from the kernel: NumPy, plain loops over (lane, frame).  Only the boxes and the what vectors are fp32 words; everything computed from
them is float64, and the scalars are the fp32 values the struct holds.  ``tables(..., ft=np.float32)`` is the fp32 restatement of the three compared
quantities (IoU, dc2, dw) the fragility band is measured with; a run given ``tol`` also says, per lane, the first frame on which a
decisive compare lies inside that band (``fragile_from``)."""
import collections

import numpy as np

from tests import score_ref as R

COUNTS = ("frames", "frames_invalid", "objects", "kept", "bridged", "reidentified", "born", "ended")
MEMORY = ("trk_id", "trk_word", "trk_age", "trk_len", "trk_box", "trk_what", "next_id", "counts")
BORN, KEPT, BRIDGED, REID = 0, 1, 2, 3

Identity = collections.namedtuple("Identity", "lane_id how track_len mem fragile_from")
Tol = collections.namedtuple("Tol", "iou dc2 dw")   # absolute errors: what each quantity is compared with is of its own size


def fresh_memory(B, M, nw, appearance=True):
    """The memory a caller starts with: trk_id = -1, everything else 0 (``appearance`` False: no trk_what)."""
    mem = dict(trk_id=-np.ones((B, M), np.int32), trk_word=np.zeros((B, M), np.int32), trk_age=np.zeros((B, M), np.int32),
               trk_len=np.zeros((B, M), np.int32), trk_box=np.zeros((B, M, 4), np.float32), next_id=np.zeros(B, np.int32),
               counts=np.zeros((B, len(COUNTS)), np.int64))
    mem["trk_what"] = np.zeros((B, M, nw), np.float32) if appearance else None
    return mem


def _centres(box, ft):
    box = np.asarray(box, ft)
    return box[..., 0] + ft(0.5) * box[..., 2], box[..., 1] + ft(0.5) * box[..., 3]


def tables(trk_box, box, trk_what, what, ft=np.float64):
    """IoU, dc2 [..., M, N] and dw [..., M, N] (None without trk_what) of every entry [..., M, .] with every slot [..., N, .] of a
    (frame, lane), in ``ft``."""
    iou = R._iou(np.asarray(trk_box, np.float32)[..., :, None, :], np.asarray(box, np.float32)[..., None, :, :], ft)
    (ty, tx), (cy, cx) = _centres(trk_box, ft), _centres(box, ft)
    dy, dx = cy[..., None, :] - ty[..., :, None], cx[..., None, :] - tx[..., :, None]
    dc2 = (dy * dy + dx * dx).astype(ft)
    dw = None
    if trk_what is not None:
        d = np.asarray(what, ft)[..., None, :, :] - np.asarray(trk_what, ft)[..., :, None, :]
        if ft is np.float32:   # the device's order: one accumulator, c in index order
            acc = np.zeros(d.shape[:-1], np.float32)
            for c in range(d.shape[-1]):
                acc = (d[..., c] * d[..., c] + acc).astype(np.float32)
            dw = (acc / np.float32(d.shape[-1])).astype(np.float32)
        else:
            dw = (d * d).sum(-1) / d.shape[-1]
    return iou, dc2, dw


def _link(iou, live, pres, words, keep, iou_min):
    """Point 2 for one (frame, lane), sq_assign_keep_greedy as the score's points 2 and 3 state it: iou [M, N] -> match [M] (j or -1)."""
    M, N = iou.shape
    ok = live[:, None] & pres[None, :] & (iou >= iou_min)   # (a NaN fails)
    match = -np.ones(M, np.int64)
    claimed = np.zeros(N, bool)
    for e in range(M):   # keep
        if keep[e] < 0:
            continue
        for j in range(N):
            if not claimed[j] and words[j] == keep[e] and ok[e, j]:
                match[e], claimed[j] = j, True
                break
    while True:          # rest: greedy; the first maximum of a row-major scan = ties to the smallest e, then the smallest j
        cand = ok & (match < 0)[:, None] & ~claimed[None, :]
        if not cand.any():
            break
        e, j = np.unravel_index(np.argmax(np.where(cand, iou, -1.0)), iou.shape)
        match[e], claimed[j] = j, True
    return match


def _fragile(iou, dc2, dw, live, pres, age, c, tol):
    """Whether a decisive compare of this (frame, lane) lies inside the band ``tol``: a candidate IoU at iou_min; two candidate pairs
    that share an entry or a slot, both (nearly) passing, nearly equal and not both exactly 1; with re-identification on, over every
    live entry x present slot (whether or not the walk reaches the pair: the conservative side), dc2 at r * r, dw at reid_what, and two
    entries nearly equal in the ranking key of one slot."""
    cand = live[:, None] & pres[None, :]
    if (cand & (np.abs(iou - c["iou_min"]) <= tol.iou)).any():
        return True
    pairs = np.argwhere(cand & (iou >= c["iou_min"] - tol.iou))
    for a in range(len(pairs)):
        for b in range(a + 1, len(pairs)):
            (e1, j1), (e2, j2) = pairs[a], pairs[b]
            if (e1 == e2 or j1 == j2) and abs(iou[e1, j1] - iou[e2, j2]) <= tol.iou and not (iou[e1, j1] == 1.0 and iou[e2, j2] == 1.0):
                return True
    if not c["reid_dist"] > 0.0:
        return False
    r2 = (c["reid_dist"] * (age.astype(np.float64) + 1.0)) ** 2
    if (cand & (np.abs(dc2 - r2[:, None]) <= tol.dc2)).any():
        return True
    if dw is not None and np.isfinite(c["reid_what"]) and (cand & (np.abs(dw - c["reid_what"]) <= tol.dw)).any():
        return True
    key, band = (dw, tol.dw) if dw is not None else (dc2, tol.dc2)
    gate = cand & (dc2 <= r2[:, None] + tol.dc2)
    for j in range(iou.shape[1]):
        es = np.flatnonzero(gate[:, j])
        for a in range(len(es)):
            for b in range(a + 1, len(es)):
                if abs(key[es[a], j] - key[es[b], j]) <= band:
                    return True
    return False


def identity(box, presence, obj_id, what, best_row, iou_min, reid_dist, reid_what, M, max_age, mem=None, appearance=True, tol=None):
    """The header's points for a pass of T frames: box [T, B, N, 4], presence, obj_id [T, B, N], what [T, B, N, nw], best_row [T, B].
    ``mem``: the memory to continue from (fresh_memory's layout; default: a fresh one); the returned one is a new dict.  ``tol``
    (a Tol): also returns fragile_from [B], each lane's first frame with a decisive compare inside the band (T where none is)."""
    T, B, N = np.asarray(presence).shape
    nw = np.asarray(what).shape[-1]
    c = dict(iou_min=float(np.float32(iou_min)), reid_dist=float(np.float32(reid_dist)), reid_what=float(np.float32(reid_what)))
    mem = fresh_memory(B, M, nw, appearance) if mem is None else {k: (None if v is None else np.array(v)) for k, v in mem.items()}
    use_what = mem["trk_what"] is not None
    words = R.words(obj_id)
    lane_id, how, track_len = (-np.ones((T, B, N), np.int32) for _ in range(3))
    first = np.full(B, T, np.int64)
    C = {n: i for i, n in enumerate(COUNTS)}
    for b in range(B):
        tid, word, age, ln, tbox, cnt = (mem[k][b] for k in ("trk_id", "trk_word", "trk_age", "trk_len", "trk_box", "counts"))
        twhat = mem["trk_what"][b] if use_what else None
        for t in range(T):
            if best_row[t, b] == -1:                       # 0: a non-finite lane
                cnt[C["frames_invalid"]] += 1
                continue
            pres = np.asarray(presence[t, b]) != 0
            live = tid >= 0
            iou, dc2, dw = tables(tbox, box[t, b], twhat, what[t, b])   # 1 (the entries outside live x pres are never used)
            if tol is not None and first[b] == T and _fragile(iou, dc2, dw, live, pres, age, c, tol):
                first[b] = t
            match = _link(iou, live, pres, words[t, b], np.where(live, word, -1), c["iou_min"])   # 2
            entry = -np.ones(N, np.int64)                  # per slot: its entry
            for e in range(M):
                if match[e] >= 0:
                    j = match[e]
                    entry[j], how[t, b, j] = e, (KEPT if word[e] == words[t, b, j] else BRIDGED)
            if c["reid_dist"] > 0.0:                       # 4
                for j in range(N):
                    if not pres[j] or entry[j] >= 0:
                        continue
                    best = None
                    for e in range(M):
                        if not live[e] or match[e] >= 0:
                            continue
                        r = c["reid_dist"] * (float(age[e]) + 1.0)
                        if not dc2[e, j] <= r * r:
                            continue
                        if use_what and not dw[e, j] <= c["reid_what"]:
                            continue
                        key = dw[e, j] if use_what else dc2[e, j]
                        if best is None or key < best[0]:
                            best = (key, e)
                    if best is not None:
                        e = best[1]
                        match[e], entry[j], how[t, b, j] = j, e, REID
            for j in range(N):                             # 5
                e = entry[j]
                if e >= 0:
                    age[e] = 0
                    ln[e] += 1
            for j in range(N):                             # 6
                if not pres[j] or entry[j] >= 0:
                    continue
                free = np.flatnonzero(tid < 0)
                if len(free):
                    e = free[0]
                else:
                    un = np.flatnonzero(match < 0)
                    e = un[np.argmax(age[un])]             # (the first of the largest ages)
                    cnt[C["ended"]] += 1
                tid[e], age[e], ln[e] = mem["next_id"][b], 0, 1
                mem["next_id"][b] += 1
                match[e], entry[j], how[t, b, j] = j, e, BORN
            for j in range(N):                             # 5, 6: the words of every seen slot
                e = entry[j]
                if e >= 0:
                    word[e], tbox[e] = words[t, b, j], box[t, b, j]
                    if use_what:
                        twhat[e] = what[t, b, j]
                    lane_id[t, b, j], track_len[t, b, j] = tid[e], ln[e]
            for e in range(M):                             # 7
                if tid[e] >= 0 and match[e] < 0:
                    age[e] += 1
                    if age[e] > max_age:
                        tid[e] = -1
                        cnt[C["ended"]] += 1
            cnt[C["frames"]] += 1                          # 8
            cnt[C["objects"]] += int(pres.sum())
            for n, v in (("born", BORN), ("kept", KEPT), ("bridged", BRIDGED), ("reidentified", REID)):
                cnt[C[n]] += int((how[t, b] == v).sum())
    return Identity(lane_id, how, track_len, mem, first)


def measured_tol(box, best_row, what, trk_what=True):
    """Four times the worst absolute error of the fp32 restatement of IoU, dc2 and dw against float64, over every pair of boxes / what
    vectors of consecutive frames of a lane -- what a track entry and a slot can hold (frames with best_row == -1 left out)."""
    ok = (np.asarray(best_row) != -1)[:, :, None, None]                     # (a non-finite lane's frame is never read)
    box, what = np.where(ok, np.asarray(box, np.float32), np.float32(0)), np.where(ok, np.asarray(what, np.float32), np.float32(0))
    T, B, N = box.shape[:3]
    prev, cur = box[:-1].reshape(-1, N, 4), box[1:].reshape(-1, N, 4)      # frame t - 1's slots against frame t's, lane by lane
    wp, wc = what[:-1].reshape(len(prev), N, -1), what[1:].reshape(len(cur), N, -1)
    err = [0.0, 0.0, 0.0]
    for s in range(0, len(prev), 64):
        k = slice(s, s + 64)
        a32 = tables(prev[k], cur[k], wp[k] if trk_what else None, wc[k], np.float32)
        a64 = tables(prev[k], cur[k], wp[k] if trk_what else None, wc[k], np.float64)
        for i in range(3 if trk_what else 2):
            err[i] = max(err[i], float(np.abs(a32[i].astype(np.float64) - a64[i]).max()))
    return Tol(*(4.0 * e for e in err))
