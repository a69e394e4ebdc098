"""The reference of track log stitching (include/sqair_hip.h: sqair_lane_tracklog_stitch, the track log stitching paragraph), restated
from the header and not from the kernel, on top of tests/tracklog_ref.py (``smooth``, ``predict``).  NumPy, plain loops.

Points 1 and 2 are integers.  Point 3, the distance of a candidate, is computed twice from the reference's own solve: in float64 from
its float64 states, and as the fp32 RESTATEMENT (numpy ``float32``, the header's operations in the header's order, ``motion_ref._fma``
where the header says ``fmaf``) from its fp32 states -- what the two differ by is the measured fp32 error of that pair's d2, the solve's
own fp32 error included.  Every decision is taken in float64: eligibility, the weights, the assignment (SciPy's
``linear_sum_assignment`` on the header's integer table, as tests/match_ref.py).  ``undecided`` counts what fp32 may decide otherwise:
the candidates whose float64 d2 lies within four times that pair's restatement error of gate^2 -- or whose determinant is within
four times its error of 0 --, plus 1 if a second-best assignment comes within the summed quantisation error of the optimum (every
other assignment lacks a pair of the optimum or weighs less: the optimum of the table without that pair, for every pair in turn;
``second_brute`` tries every partial assignment for small tables).  The cases are chosen so that it is 0.

Point 6 by its definition: the stitched table is ``tracklog_ref.smooth`` of the log in which every kept fragment carries its chain's
root id and every other id of the window is gone (the solve would keep them otherwise: a stitched table has one column per chain of
KEPT fragments), with n_tracks = the solve's minus the links; ``work_out`` is ``tracklog_fit_ref.slots`` of that."""
import collections

import numpy as np
from scipy.optimize import linear_sum_assignment

from tests import tracklog_fit_ref as FR
from tests import tracklog_ref as R

UNIT = 1048576.0
BIG = 1 << 28

Cand = collections.namedtuple("Cand", "a c gap steps d2 d2_32 det det32 err det_err eligible")
Stitch = collections.namedtuple("Stitch", "link_next link_d2 link_d2_32 link_gap root n_links table work_out cands undecided d2_err log")


def spans(state, b):
    """Point 1 for lane b: (f0 [C], f1 [C]) of the columns' frames with state != 0 (lag and -1 for a column without one)."""
    lag, _, C = state.shape
    f0, f1 = np.full(C, lag), np.full(C, -1)
    for c in range(C):
        on = np.flatnonzero(state[:, b, c] != 0)
        if len(on):
            f0[c], f1[c] = on[0], on[-1]
    return f0, f1


def d2_axis(fa, sb, steps, q, r, ft):
    """Point 3 for one axis in ``ft``: (d2_axis, det) from the predecessor's five filtered words and the successor's five smoothed."""
    fma = R._fmaf(ft)
    k = [ft(v) for v in fa]
    for _ in range(steps):
        k, _S = R.predict(k, q, r, ft)
    s = [ft(v) for v in sb]
    A, Bm, Cm = k[2] + s[2], k[3] + s[3], k[4] + s[4]
    det = fma(A, Cm, -(Bm * Bm))
    dp, dv = s[0] - k[0], s[1] - k[1]
    num = fma(A * dv, dv, fma(ft(-2), Bm * dv, Cm * dp) * dp)
    return num / det, det


def d2_pair(fa, sb, steps, q, r, ft):
    """(d2, the smaller det) of both axes: fa, sb [2, 5]."""
    (y, dy), (x, dx) = d2_axis(fa[0], sb[0], steps, q, r, ft), d2_axis(fa[1], sb[1], steps, q, r, ft)
    return y + x, min(dy, dx) if dy == dy and dx == dx else ft(np.nan)


def weight_table(cands, C, gate2):
    """Point 4's integer table [C, C]: 2^28 + q for an eligible candidate, q rounded to nearest even as __float2int_rn, -1 elsewhere."""
    w = -np.ones((C, C), np.int64)
    for k in cands:
        if k.eligible:
            w[k.a, k.c] = BIG + int(np.clip(np.rint((1.0 - k.d2 / gate2) * UNIT), 0, UNIT))
    return w


def solve(w):
    """The optimum over all partial one-to-one assignments of the table, pairs of weight -1 never taken: (value, {a: c})."""
    rows, cols = linear_sum_assignment(np.maximum(w, 0), maximize=True)
    pairs = {int(a): int(c) for a, c in zip(rows, cols) if w[a, c] > 0}
    return int(sum(w[a, c] for a, c in pairs.items())), pairs


def second(w, pairs):
    """The best value of an assignment other than ``pairs`` (the optimum): it lacks one of its pairs (a superset would weigh more)."""
    best = -1
    for a, c in pairs.items():
        w2 = w.copy()
        w2[a, c] = -1
        best = max(best, solve(w2)[0])
    return best


def second_brute(w):
    """(the optimum, the second-best value over all DISTINCT partial assignments) by trying every one: small tables only."""
    C = w.shape[0]
    vals = []

    def go(a, used, tot):
        if a == C:
            vals.append(tot)
            return
        go(a + 1, used, tot)
        for c in range(C):
            if not used >> c & 1 and w[a, c] > 0:
                go(a + 1, used | 1 << c, tot + int(w[a, c]))
    go(0, 0, 0)
    vals.sort(reverse=True)
    return vals[0], (vals[1] if len(vals) > 1 else -1)


def relabelled(log, sm, lag, link_next):
    """The log in which, in the window's records of the frames that count, a kept id is its chain's root id and any other id is -1."""
    out = {k: np.array(v) for k, v in log.items()}
    B, C = sm.track_id.shape
    for b in range(B):
        prev = {int(link_next[b, a]): a for a in range(C) if link_next[b, a] >= 0}
        root_id = {}
        for c in range(C):
            if sm.track_id[b, c] < 0:
                continue
            r = c
            while r in prev:
                r = prev[r]
            root_id[int(sm.track_id[b, c])] = int(sm.track_id[b, r])
        _, rec, counts = R.window(log, b, lag)
        for f in range(lag):
            if counts[f]:
                ids = out["log_id"][b, rec[f]]
                out["log_id"][b, rec[f]] = [root_id.get(int(i), -1) for i in ids]
    return out


def stitch(log, sm, lag, C, q, r, v0_var, gate, max_gap):
    """Points 1 to 7 on a log {name: array} and the reference's solve of it ``sm`` (tracklog_ref.Smooth); the scalars are taken as the
    fp32 values the call is handed, gate^2 as the fp32 product."""
    q, r, v0_var = (float(np.float32(v)) for v in (q, r, v0_var))
    gate2_32 = np.float32(gate) * np.float32(gate)
    gate2 = float(gate2_32)
    B = sm.track_id.shape[0]
    link_next, link_gap = -np.ones((B, C), np.int32), -np.ones((B, C), np.int32)
    link_d2, link_d2_32 = np.zeros((B, C)), np.zeros((B, C), np.float32)
    n_links = np.zeros(B, np.int32)
    all_cands, undecided, d2_err = [], 0, 0.0
    for b in range(B):
        _, _rec, counts = R.window(log, b, lag)
        pre = np.concatenate([[0], np.cumsum(counts)])            # the counting frames below f
        f0, f1 = spans(sm.state, b)
        cands = []
        for a in range(C):
            for c in range(C):
                if a == c or sm.track_id[b, a] < 0 or sm.track_id[b, c] < 0 or not f1[a] < f0[c] or sm.len0[b, c] != 1:     # 2
                    continue
                gap = int(pre[f0[c]] - pre[f1[a] + 1])
                if gap > max_gap:
                    continue
                steps = int(pre[f0[c] + 1] - pre[f1[a] + 1])
                with np.errstate(all="ignore"):
                    d64, det64 = d2_pair(sm.filt[f1[a], b, a], sm.smooth[f0[c], b, c], steps, q, r, np.float64)                # 3
                    d32, det32 = d2_pair(sm.filt32[f1[a], b, a], sm.smooth32[f0[c], b, c], steps, q, r, np.float32)
                    err, det_err = abs(float(d32) - float(d64)), abs(float(det32) - float(det64))
                ok = bool(det64 > 0 and d64 <= gate2)             # (a NaN fails)
                cands.append(Cand(a, c, gap, steps, float(d64), np.float32(d32), float(det64), float(det32), err, det_err, ok))
                if np.isfinite(d64) and np.isfinite(err):
                    d2_err = max(d2_err, err) if ok else d2_err    # (of the eligible ones: only they become links)
                    undecided += abs(d64 - gate2) <= 4.0 * err or abs(det64) <= 4.0 * det_err
        w = weight_table(cands, C, gate2)                                                                                           # 4
        best, pairs = solve(w)
        if pairs:
            slack = sum(4.0 * k.err / gate2 * UNIT + 1.0 for k in cands if k.eligible)
            undecided += best - second(w, pairs) <= slack
        by = {(k.a, k.c): k for k in cands}
        for a, c in pairs.items():
            link_next[b, a], link_gap[b, a] = c, by[a, c].gap
            link_d2[b, a], link_d2_32[b, a] = by[a, c].d2, by[a, c].d2_32
        n_links[b] = len(pairs)
        all_cands.append(cands)
    log2 = relabelled(log, sm, lag, link_next)                                                                                 # 5, 6
    with np.errstate(all="ignore"):
        table = R.smooth(log2, lag, C, q, r, v0_var)
    table = table._replace(n_tracks=(sm.n_tracks - n_links).astype(np.int32))
    work_out = FR.slots(log2, table, lag)
    root = -np.ones((B, C), np.int32)                                                                                          # 7
    for b in range(B):
        prev = {int(link_next[b, a]): a for a in range(C) if link_next[b, a] >= 0}
        for c in range(C):
            if sm.track_id[b, c] >= 0:
                rt = c
                while rt in prev:
                    rt = prev[rt]
                root[b, c] = list(table.track_id[b]).index(sm.track_id[b, rt])
    return Stitch(link_next, link_d2, link_d2_32, link_gap, root, n_links, table, work_out, all_cands, int(undecided), d2_err, log2)


def dense_d2(fa, sb, steps, q):
    """The same distance from densely assembled covariances with numpy.linalg: per axis x = (p, v), P = [[Ppp, Ppv], [Ppv, Pvv]], the
    predecessor coasted as F^n x, F^n P F^nT + sum_i F^i Q F^iT with Q = q [[1/4, 1/2], [1/2, 1]], then d^T (Pa + Pb)^-1 d summed."""
    F = np.array([[1.0, 1.0], [0.0, 1.0]])
    Q = q * np.array([[0.25, 0.5], [0.5, 1.0]])
    tot = 0.0
    for ax in range(2):
        xa, Pa = np.array(fa[ax][:2], np.float64), np.array([[fa[ax][2], fa[ax][3]], [fa[ax][3], fa[ax][4]]], np.float64)
        Fn = np.linalg.matrix_power(F, steps)
        xa = Fn @ xa
        Pa = Fn @ Pa @ Fn.T + sum(np.linalg.matrix_power(F, i) @ Q @ np.linalg.matrix_power(F, i).T for i in range(steps))
        xb, Pb = np.array(sb[ax][:2], np.float64), np.array([[sb[ax][2], sb[ax][3]], [sb[ax][3], sb[ax][4]]], np.float64)
        d = xb - xa
        tot += float(d @ np.linalg.solve(Pa + Pb, d))
    return tot
