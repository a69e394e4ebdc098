"""The float64 reference of lane motion (include/sqair_hip.h: sqair_set_motion, the motion paragraph), restated from the header and
not from the kernel: tests/identity_ref.py's ``identity`` extended by the points P and U -- a constant-velocity filter per (entry,
axis) of the box centre --, the predicted box in point 1 and the gate d2 <= gate * gate in point 4.  NumPy, plain loops over (lane,
frame).  Only the boxes and the what vectors are fp32 words; everything computed from them is float64, the scalars are the fp32
values the structs hold.

Beside the float64 state every run carries the fp32 RESTATEMENT of the filter (numpy ``float32``, the header's operations in the
header's order, a fused multiply-add where the header's update is one: ``_fma``), driven by the float64 run's decisions so that it
never leaves its path.  What it differs by from float64 is the measured fp32 error of every compared quantity: ``Motion.err`` holds,
over all lanes, the worst error of IoU, d2 and dw over candidate pairs (d2: over the pairs with d2 <= 2 gate^2 -- the error of d2 is
relative, and only values near gate^2 are ever compared with it or ranked) and, per lane, the worst error of velocity, nis and the
final state of the live entries.  ``fragile_from(m, tol)``: each lane's first frame with a decisive compare inside the band ``tol``,
from the margins the run recorded."""
import collections

import numpy as np

from tests import identity_ref as IR
from tests import match_ref as MR
from tests import score_ref as R

BORN, KEPT, BRIDGED, REID = IR.BORN, IR.KEPT, IR.BRIDGED, IR.REID
COUNTS = IR.COUNTS
STATE = ("p", "v", "Ppp", "Ppv", "Pvv")
PRE_IOU, PRE_D2 = 1e-3, 1e-2      # how near a pair must come to a threshold for its ties to be looked at: far wider than any band

Motion = collections.namedtuple("Motion", "lane_id how track_len velocity nis mem margins err")
Tol = collections.namedtuple("Tol", "iou d2 dw")
Scalars = collections.namedtuple("Scalars", "q r v0_var gate")


def fresh_memory(B, M, nw, appearance=True):
    """identity_ref's memory with the filter's state: trk_kf [B, M, 2, 5] float64 and its fp32 restatement trk_kf32, zeros."""
    mem = IR.fresh_memory(B, M, nw, appearance)
    mem["trk_kf"], mem["trk_kf32"] = np.zeros((B, M, 2, 5), np.float64), np.zeros((B, M, 2, 5), np.float32)
    return mem


def _fma(a, b, c):
    """fmaf on float32 operands: the product of two floats is exact in float64."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def predict(k, live, s, ft):
    """Point P in place on k [M, 2, 5] for the live entries, in ``ft``; returns S [M, 2] (whatever for the others)."""
    q, r = ft(s.q), ft(s.r)
    p, v, a, b, c = (k[..., i].copy() for i in range(5))
    new = np.stack([p + v, v, ((a + ft(2) * b) + c) + ft(0.25) * q, (b + c) + ft(0.5) * q, c + q], -1).astype(ft)
    k[live] = new[live]
    return (k[..., 2] + r).astype(ft)


def update(k, S, z, ft):
    """Point U for one (entry, axis): k [5] predicted -> posterior, in place, in ``ft``."""
    p, v, a, b, c = (ft(x) for x in k)
    y, k0, k1 = z - p, a / S, b / S
    if ft is np.float32:
        k[:] = (_fma(k0, y, p), _fma(k1, y, v), (ft(1) - k0) * a, (ft(1) - k0) * b, _fma(-k1, b, c))
    else:
        k[:] = (p + k0 * y, v + k1 * y, (1.0 - k0) * a, (1.0 - k0) * b, c - k1 * b)


def centres(box, ft):
    """(cy, cx) [N] of box [N, 4] in ``ft``: fmaf(0.5, h, y) -- 0.5 h is exact, so one rounding either way."""
    bx = np.asarray(box, ft)
    return bx[:, 0] + ft(0.5) * bx[:, 2], bx[:, 1] + ft(0.5) * bx[:, 3]


def tables(k, S, trk_box, box, ft):
    """IoU of every entry's predicted box with every slot [M, N], and d2 [M, N], in ``ft`` (free entries: whatever)."""
    tb = np.asarray(trk_box, ft)
    pbox = np.stack([k[:, 0, 0] - ft(0.5) * tb[:, 2], k[:, 1, 0] - ft(0.5) * tb[:, 3], tb[:, 2], tb[:, 3]], -1).astype(ft)
    iou = R._iou(pbox[:, None, :], np.asarray(box, np.float32)[None, :, :], ft)
    cy, cx = centres(box, ft)
    with np.errstate(all="ignore"):
        dy, dx = cy[None, :] - k[:, 0, 0][:, None], cx[None, :] - k[:, 1, 0][:, None]
        d2 = ((dy * dy) / S[:, 0][:, None] + (dx * dx) / S[:, 1][:, None]).astype(ft)
    return iou, d2, pbox


def _margins(iou, d2, dw, live, pres, c, optimal, words, keep):
    """How far the decisive compares of this (frame, lane) are from flipping: [iou, d2, dw, opt] -- the least |IoU - iou_min| over
    candidates and the least difference of two candidate IoUs that share an entry or a slot and both (nearly) pass, not both exactly
    1 (greedy mode; in optimal mode ``opt``: by how many units of q per pair the best assignment that differs from the optimum falls
    short of it, beyond the rounding of q -- tests/match_ref.py's slack solved for e); with re-identification on, over every live
    entry x present slot, the least |d2 - gate^2| and |dw - reid_what|, and the least difference in the ranking key of two
    entries (nearly) inside the gate of one slot."""
    m = [np.inf, np.inf, np.inf, np.inf]
    cand = live[:, None] & pres[None, :]
    if not cand.any():
        return m
    m[0] = float(np.abs(iou - c["iou_min"])[cand].min())
    near = cand & (iou >= c["iou_min"] - PRE_IOU)
    pairs = np.argwhere(near)
    if optimal:
        if len(pairs) > 1 and (len(set(pairs[:, 0])) < len(pairs) or len(set(pairs[:, 1])) < len(pairs)):
            ok = cand & (iou >= c["iou_min"])
            kept, claimed = MR.keep_step(ok, words, keep)
            w = MR.weights(iou, ok, kept, claimed)
            value, best = MR.solve(w)
            for g, j in best:      # the best assignment without this pair: the runner-up is one of these
                w2 = w.copy()
                w2[g, j] = -1
                other = MR.solve(w2)[0]
                if value - other < MR.BIG // 2:      # (the same number of pairs)
                    m[3] = min(m[3], max((value - other) / (2.0 * max(len(best), 1)) - 1.0, 0.0))
    else:
        for a in range(len(pairs)):
            for b in range(a + 1, len(pairs)):
                (e1, j1), (e2, j2) = pairs[a], pairs[b]
                if (e1 == e2 or j1 == j2) and not (iou[e1, j1] == 1.0 and iou[e2, j2] == 1.0):
                    m[0] = min(m[0], abs(iou[e1, j1] - iou[e2, j2]))
    if not c["reid_dist"] > 0.0:
        return m
    g2 = c["gate"] ** 2
    with np.errstate(invalid="ignore"):
        m[1] = float(np.abs(d2 - g2)[cand].min())
        if dw is not None and np.isfinite(c["reid_what"]):
            m[2] = float(np.abs(dw - c["reid_what"])[cand].min())
        gate = cand & (d2 <= g2 + PRE_D2)
    key, ki = (dw, 2) if dw is not None else (d2, 1)
    for j in range(iou.shape[1]):
        ks = np.sort(key[gate[:, j], j])
        if len(ks) > 1:
            m[ki] = min(m[ki], float(np.diff(ks).min()))
    return m


def fragile_from(margins, tol):
    """[B]: each lane's first frame with a margin inside the band (T where none is).  margins [T, B, 4]; the optimal mode's margin is
    in units of q = 2^-20 of IoU."""
    T = margins.shape[0]
    band = np.array([tol.iou, tol.d2, tol.dw, tol.iou * MR.UNIT])
    near = (margins <= band).any(-1)
    return np.where(near.any(0), near.argmax(0), T).astype(np.int64)


def identity(box, presence, obj_id, what, best_row, iou_min, reid_dist, reid_what, M, max_age, motion, mem=None, appearance=True,
             optimal=False):
    """identity_ref.identity's arguments and ``motion`` = Scalars(q, r, v0_var, gate): the motion paragraph for a pass of T frames.
    Returns the identity's outputs, velocity [T, B, N, 2] and nis [T, B, N] (float64), the memory, the margins [T, B, 4] of
    ``_margins`` and the measured errors (the module's docstring)."""
    T, B, N = np.asarray(presence).shape
    nw = np.asarray(what).shape[-1]
    s = Scalars(*(float(np.float32(v)) for v in motion))
    c = dict(iou_min=float(np.float32(iou_min)), reid_dist=float(np.float32(reid_dist)), reid_what=float(np.float32(reid_what)), gate=s.gate)
    mem = fresh_memory(B, M, nw, appearance) if mem is None else {k: (None if v is None else np.array(v)) for k, v in mem.items()}
    use_what = mem["trk_what"] is not None
    link = MR.link if optimal else IR._link
    words = R.words(obj_id)
    lane_id, how, track_len = (-np.ones((T, B, N), np.int32) for _ in range(3))
    velocity, nis = np.zeros((T, B, N, 2)), np.zeros((T, B, N))
    margins = np.full((T, B, 4), np.inf)
    err = dict(iou=0.0, d2=0.0, dw=0.0, velocity=np.zeros(B), nis=np.zeros(B), kf=np.zeros(B))
    C = {n: i for i, n in enumerate(COUNTS)}
    f32 = np.float32
    for b in range(B):
        tid, word, age, ln, tbox, cnt = (mem[k][b] for k in ("trk_id", "trk_word", "trk_age", "trk_len", "trk_box", "counts"))
        twhat = mem["trk_what"][b] if use_what else None
        kf, k32 = mem["trk_kf"][b], mem["trk_kf32"][b]
        for t in range(T):
            if best_row[t, b] == -1:                       # a non-finite lane: no predict, no ageing
                cnt[C["frames_invalid"]] += 1
                continue
            pres = np.asarray(presence[t, b]) != 0
            live = tid >= 0
            S, S32 = predict(kf, live, s, np.float64), predict(k32, live, s, f32)                        # P
            iou, d2, _ = tables(kf, S, tbox, box[t, b], np.float64)                                      # 1, 4's tables
            dw = IR.tables(tbox, box[t, b], twhat, what[t, b])[2] if use_what and c["reid_dist"] > 0.0 else None
            cand = live[:, None] & pres[None, :]
            if cand.any():                                 # the fp32 restatement's error of what is compared
                iou32, d232, _ = tables(k32, S32, tbox, box[t, b], f32)
                err["iou"] = max(err["iou"], float(np.abs(iou32 - iou)[cand].max()))
                sel = cand & (d2 <= 2.0 * s.gate ** 2)
                if sel.any():
                    err["d2"] = max(err["d2"], float(np.abs(d232 - d2)[sel].max()))
                if dw is not None:
                    dw32 = IR.tables(tbox, box[t, b], twhat, what[t, b], f32)[2]
                    err["dw"] = max(err["dw"], float(np.abs(dw32 - dw)[cand].max()))
            keep = np.where(live, word, -1)
            margins[t, b] = _margins(iou, d2, dw, live, pres, c, optimal, words[t, b], keep)
            match = link(iou, live, pres, words[t, b], keep, c["iou_min"])                               # 2
            entry = -np.ones(N, np.int64)
            for e in range(M):
                if match[e] >= 0:
                    j = match[e]
                    entry[j], how[t, b, j] = e, (KEPT if word[e] == words[t, b, j] else BRIDGED)
            if c["reid_dist"] > 0.0:                       # 4: the gate is the filter's
                for j in range(N):
                    if not pres[j] or entry[j] >= 0:
                        continue
                    best = None
                    for e in range(M):
                        if not live[e] or match[e] >= 0:
                            continue
                        if not d2[e, j] <= s.gate * s.gate:
                            continue
                        if use_what and not dw[e, j] <= c["reid_what"]:
                            continue
                        key = dw[e, j] if use_what else d2[e, j]
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
                    e = un[np.argmax(age[un])]
                    cnt[C["ended"]] += 1
                tid[e], age[e], ln[e] = mem["next_id"][b], 0, 1
                mem["next_id"][b] += 1
                match[e], entry[j], how[t, b, j] = j, e, BORN
            cy, cx = centres(box[t, b], np.float64)
            cy32, cx32 = centres(box[t, b], f32)
            for j in range(N):                             # U, and 5, 6: the words of every seen slot
                e = entry[j]
                if e < 0:
                    continue
                for ax, (z, z32) in enumerate(((cy[j], cy32[j]), (cx[j], cx32[j]))):
                    if how[t, b, j] == BORN:
                        kf[e, ax] = (z, 0.0, s.r, 0.0, s.v0_var)
                        k32[e, ax] = (z32, 0.0, s.r, 0.0, s.v0_var)
                    else:
                        update(kf[e, ax], S[e, ax], z, np.float64)
                        update(k32[e, ax], S32[e, ax], z32, f32)
                        velocity[t, b, j, ax] = kf[e, ax, 1]
                        err["velocity"][b] = max(err["velocity"][b], abs(float(k32[e, ax, 1]) - kf[e, ax, 1]))
                if how[t, b, j] != BORN:
                    nis[t, b, j] = d2[e, j]
                    err["nis"][b] = max(err["nis"][b], abs(float(d232[e, j]) - d2[e, j]))
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
        if (tid >= 0).any():
            err["kf"][b] = float(np.abs(k32.astype(np.float64) - kf)[tid >= 0].max())
    return Motion(lane_id, how, track_len, velocity, nis, mem, margins, err)


def measured_tol(err):
    """The fragility band: four times the measured error of the fp32 restatement of each compared quantity."""
    return Tol(4.0 * err["iou"], 4.0 * err["d2"], 4.0 * err["dw"])


def bars(err, lanes):
    """The bars of velocity, nis and trk_kf: four times the largest error of the fp32 restatement over ``lanes`` [B] bool."""
    return {n: 4.0 * float(err[n][lanes].max()) if lanes.any() else 0.0 for n in ("velocity", "nis", "kf")}


def steady_state(q, r):
    """The closed-form steady state of one axis seen every frame, F = [[1, 1], [0, 1]], Q = q [[1/4, 1/2], [1/2, 1]]: the alpha-beta
    filter's gains (Kalata's tracking index lam = sqrt(q / r)), (k0, k1)."""
    lam = np.sqrt(q / r)
    rr = (4.0 + lam - np.sqrt(8.0 * lam + lam * lam)) / 4.0
    alpha = 1.0 - rr * rr
    beta = 2.0 * (2.0 - alpha) - 4.0 * np.sqrt(1.0 - alpha)
    return alpha, beta


# ---- the hand-made scenarios of tests/motion_cases.py: one object, one entry, no appearance --------------------------------------
SCENARIO = dict(iou_min=0.3, reid_what=float("inf"), M=1, appearance=False)


def scenario_run(x, reid_dist, max_age, motion, frames=None):
    """The reference on a scenario's inputs (their first ``frames`` frames)."""
    x = x if frames is None else {k: v[:frames] for k, v in x.items()}
    return identity(reid_dist=reid_dist, max_age=max_age, motion=motion, **SCENARIO, **x)


def scenario_plain(x, reid_dist, max_age):
    """tests/identity_ref.py on the same inputs: what the stream says without the feature."""
    return IR.identity(reid_dist=reid_dist, max_age=max_age, **SCENARIO, **x)


def predicted_iou(x, t, reid_dist, max_age, motion):
    """The IoU of the track's predicted box with the slot's box in frame t of a scenario: the state after frames 0 .. t - 1, one
    predict step on."""
    mem = scenario_run(x, reid_dist, max_age, motion, frames=t).mem
    k = mem["trk_kf"][0].copy()
    predict(k, mem["trk_id"][0] >= 0, Scalars(*motion), np.float64)
    size = mem["trk_box"][0, 0, 2:].astype(np.float64)
    return float(R.iou64(np.concatenate([k[0, :, 0] - 0.5 * size, size]), x["box"][t, 0, 0]))
