"""Two references of HOTA scoring (include/sqair_hip.h: sqair_set_hota), neither restated from the kernels.

``hota_float``: the published algorithm (Luiten et al., IJCV 2020, as TrackEval computes it) in float64 with SciPy's
linear_sum_assignment: the per-frame similarity normalised by everything either side overlaps, the global alignment score from its
sum over the clip, one assignment per frame on alignment x similarity, the nineteen thresholds 0.05 .. 0.95 on the matched pairs.

``solve`` / ``solve_lane``: the header's integer statement, points 3 to 6, in Python ints on a clip log, and ``append``: its points 1
and 2, the log itself, from float64 IoUs of the fp32 box words (tests/score_ref.py: iou_table).  ``append`` can hand out the float64
similarities of the records it writes, so that both references run on the very same frames, columns and dropped frames.

Optimal assignments tie and the header states no rule among them: ``judge`` holds a given matching to feasibility and to SciPy's
optimum of the integer table exactly, and ``solve`` takes a matching to impose."""
import numpy as np
from scipy.optimize import linear_sum_assignment

from tests import score_ref as SR

ALPHAS = 19
UNIT = 1 << 20
A = [-(-(i * UNIT) // 20) for i in range(1, ALPHAS + 1)]      # ceil(i 2^20 / 20): A[9] = 2^19
INT, FLOAT, CLIP = ("tp", "fn", "fp", "loc"), ("ass", "assre", "asspr"), ("clips", "frames", "dropped_frames", "overflow_ids")
LOG = ("col_id", "log_q", "log_col", "log_row", "frames", "dropped_frames")
TOTALS = ("totals_i", "totals_f", "totals_c")
NOTE = ("statement_vs_float: the header's integer statement of HOTA against the published algorithm in float64 on the clips of "
        "tests/hota_cases.py (CPU); device_vs_scipy: the share of records where the device's matching is not SciPy's own and the HOTA "
        "difference that makes (tests/test_hota_solve_kernel.py, recorded, not gated)")


def fresh_parity():
    """hota_parity.json before its first case: tests/test_hota_ref.py and tests/test_hota_solve_kernel.py write the same file."""
    return {"note": NOTE, "statement_vs_float": {}, "device_vs_scipy": {}}


# ------------------------------------------------------------------------------------------------ the log (points 1 and 2)
def new_log(B, G, N, P, L):
    """A fresh log {name: array} with its totals: col_id -1, the counters 0; the records hold -7 (never read)."""
    return dict(col_id=-np.ones((B, P), np.int32), log_q=np.full((B, L, G, N), -7, np.int32), log_col=np.full((B, L, N), -7, np.int32),
                log_row=np.full((B, L), -7, np.int32), frames=np.zeros(B, np.int32), dropped_frames=np.zeros(B, np.int32),
                totals_i=np.zeros((B, ALPHAS, 4), np.int64), totals_f=np.zeros((B, ALPHAS, 3), np.float64), totals_c=np.zeros((B, 4), np.int64))


def copy_log(t):
    return {n: np.array(v) for n, v in t.items()}


def append(log, box, presence, ids, map_count, truth_box, truth_present, truth_valid, sims=None):
    """Points 1 and 2 for a pass of T frames, continuing ``log`` (a new one is returned): box [T, B, N, 4], presence, ids [T, B, N]
    (int32 words), map_count [T, B]; truth_box [T, B, G, 4], truth_present [T, B, G], truth_valid [T, B].  ``sims``: a list of B lists
    that receives, per record taken, its float64 similarities [G, N] (NaN where the log holds -1)."""
    t = copy_log(log)
    T, B, G = np.asarray(truth_present).shape
    N = np.asarray(presence).shape[2]
    P, L = t["col_id"].shape[1], t["log_row"].shape[1]
    iou = SR.iou_table(truth_box, box)
    for b in range(B):
        for f in range(T):
            if truth_valid[f, b] == 0 or map_count[f, b] == -1:
                continue
            if t["frames"][b] >= L:
                t["dropped_frames"][b] += 1
                continue
            r = int(t["frames"][b])
            t["frames"][b] += 1
            col = -np.ones(N, np.int64)
            for j in range(N):
                if presence[f, b, j] == 0:
                    continue
                word, c = int(ids[f, b, j]), -2
                if word >= 0:
                    hit = np.flatnonzero(t["col_id"][b] == word)
                    free = np.flatnonzero(t["col_id"][b] < 0)
                    if hit.size:
                        c = int(hit[0]) if int(hit[0]) not in col[:j] else -2
                    elif free.size:
                        c = int(free[0])
                        t["col_id"][b, c] = word
                col[j] = c
            t["totals_c"][b, 3] += bool((col == -2).any())
            pair = (np.asarray(truth_present[f, b]) != 0)[:, None] & (col >= 0)[None, :]
            with np.errstate(invalid="ignore"):
                t["log_q"][b, r] = np.where(pair, np.rint(np.where(pair, iou[f, b], 0.0) * UNIT), -1).astype(np.int32)
            t["log_col"][b, r] = col
            t["log_row"][b, r] = sum(1 << g for g in range(G) if truth_present[f, b, g] != 0)
            if sims is not None:
                sims[b].append(np.where(pair, iou[f, b], np.nan))
    return t


def records(log, b):
    """Lane b's records in use: [(q [G, N], col [N], row word)]."""
    return [(log["log_q"][b, r], log["log_col"][b, r], int(log["log_row"][b, r])) for r in range(int(log["frames"][b]))]


# ------------------------------------------------------------------------------------------------ the integer statement (points 3-6)
def best_assignment(w):
    """SciPy's optimum over partial one-to-one assignments of the integer table w (a pair of negative weight is never taken): (value,
    match [G] of j or -1).  A pair of weight 0 that SciPy's full assignment holds is kept, as the published algorithm keeps it."""
    w = np.asarray(w, np.int64)
    m = -np.ones(w.shape[0], np.int64)
    rows, cols = linear_sum_assignment(np.maximum(w, 0), maximize=True)
    for g, j in zip(rows, cols):
        if w[g, j] >= 0:
            m[g] = j
    return int(sum(w[g, m[g]] for g in range(len(m)) if m[g] >= 0)), m


def judge(w, m):
    """A given matching m [G] on the table w: one-to-one, only pairs of weight >= 0, its total SciPy's optimum exactly."""
    w = np.asarray(w, np.int64)
    pairs = [(g, int(j)) for g, j in enumerate(m) if j >= 0]
    cols = [j for _, j in pairs]
    assert len(set(cols)) == len(cols), ("not one-to-one", m)
    assert all(0 <= j < w.shape[1] and w[g, j] >= 0 for g, j in pairs), ("a pair of negative weight", m, w)
    assert sum(int(w[g, j]) for g, j in pairs) == best_assignment(w)[0], ("not optimal", m, w)


def alignment(recs, G, P):
    """Pass 1: (gas [G][P] ints in units of 2^-20, row_frames [G], col_frames [P], extra)."""
    pot = [[0] * P for _ in range(G)]
    rf, cf, extra = [0] * G, [0] * P, 0
    for q, col, row in recs:
        q = [[int(v) for v in qg] for qg in q]
        N = len(col)
        R = [sum(v for v in q[g] if v >= 0) for g in range(G)]
        C = [sum(q[g][j] for g in range(G) if q[g][j] >= 0) for j in range(N)]
        for g in range(G):
            rf[g] += row >> g & 1
            for j in range(N):
                if q[g][j] >= 0:
                    den = R[g] + C[j] - q[g][j]
                    pot[g][int(col[j])] += (q[g][j] << 20) // den if den else 0
        for j in range(N):
            if col[j] >= 0:
                cf[int(col[j])] += 1
            extra += col[j] == -2
    gas = [[0] * P for _ in range(G)]
    for g in range(G):
        for p in range(P):
            den = ((rf[g] + cf[p]) << 20) - pot[g][p]
            gas[g][p] = (pot[g][p] << 20) // den if den else 0
    return gas, rf, cf, int(extra)


def weights(gas, q, col):
    """Pass 2's table of one record: (gas q) >> 15 for the pairs with q >= 0, -1 elsewhere."""
    G, N = np.asarray(q).shape
    return np.array([[(gas[g][int(col[j])] * int(q[g][j])) >> 15 if q[g][j] >= 0 else -1 for j in range(N)] for g in range(G)], np.int64)


def solve_lane(recs, G, P, match=None):
    """Points 3 to 5 for one lane's records: ints [19, 4] int64 (tp, fn, fp, loc), floats [19, 3] float64 (ass, assre, asspr), the
    matchings [F, G] and the tables they were made on.  ``match`` [F, G]: imposed (else SciPy's own)."""
    gas, rf, cf, extra = alignment(recs, G, P)
    tp, loc = [0] * ALPHAS, [0] * ALPHAS
    mc = np.zeros((ALPHAS, G, P), np.int64)
    matches, tables = -np.ones((len(recs), G), np.int64), []
    for r, (q, col, _) in enumerate(recs):
        w = weights(gas, q, col)
        tables.append(w)
        m = best_assignment(w)[1] if match is None else np.asarray(match[r])
        matches[r] = m
        for g in range(G):
            if m[g] >= 0:
                qq = int(q[g][m[g]])
                for i in range(ALPHAS):
                    if qq >= A[i]:
                        tp[i] += 1
                        loc[i] += qq
                        mc[i, g, int(col[m[g]])] += 1
    ints = np.array([[tp[i], sum(rf) - tp[i], sum(cf) + extra - tp[i], loc[i]] for i in range(ALPHAS)], np.int64)
    floats = np.zeros((ALPHAS, 3), np.float64)
    for i in range(ALPHAS):
        for g in range(G):
            for p in range(P):
                m = int(mc[i, g, p])
                if m > 0:
                    floats[i] += (m * m / float(rf[g] + cf[p] - m), m * m / float(rf[g]), m * m / float(cf[p]))
    return ints, floats, matches, tables


def solve(log, close=None, match=None):
    """Points 3 to 6 for every lane: (log after, open_i [B, 19, 4], open_f [B, 19, 3], open_c [B, 4], match [B, L, G] with -9 in the
    records not in use, tables: per lane the records' weight tables).  ``match`` [B, L, G]: imposed."""
    t = copy_log(log)
    B, L, G, _ = t["log_q"].shape
    P = t["col_id"].shape[1]
    open_i, open_f = np.zeros((B, ALPHAS, 4), np.int64), np.zeros((B, ALPHAS, 3), np.float64)
    open_c, out = np.zeros((B, 4), np.int64), np.full((B, L, G), -9, np.int64)
    tables = []
    for b in range(B):
        F = int(t["frames"][b])
        open_i[b], open_f[b], m, w = solve_lane(records(t, b), G, P, None if match is None else match[b])
        out[b, :F] = m
        tables.append(w)
        open_c[b] = (F > 0, F, t["dropped_frames"][b], 0)
        if close is not None and close[b] != 0:
            t["totals_i"][b] += open_i[b]
            t["totals_f"][b] += open_f[b]
            t["totals_c"][b] += open_c[b]
            t["col_id"][b] = -1
            t["frames"][b] = t["dropped_frames"][b] = 0
    return t, open_i, open_f, open_c, out, tables


def figures(ints, floats):
    """The ratios of point 6 from (tp, fn, fp, loc) [19, 4] and (ass, assre, asspr) [19, 3]: per threshold ``hota_alpha``,
    ``deta_alpha``, ``assa_alpha`` and the means ``hota``, ``deta``, ``assa``, ``detre``, ``detpr``, ``assre``, ``asspr``, ``loca``;
    NaN without a denominator."""
    ints, floats = np.asarray(ints, np.float64), np.asarray(floats, np.float64)
    tp, fn, fp, loc = ints.T
    with np.errstate(invalid="ignore", divide="ignore"):
        div = lambda a, b: np.where(b != 0, a / np.where(b != 0, b, 1.0), np.nan)
        per = dict(deta=div(tp, tp + fn + fp), detre=div(tp, tp + fn), detpr=div(tp, tp + fp), assa=div(floats[:, 0], tp),
                   assre=div(floats[:, 1], tp), asspr=div(floats[:, 2], tp), loca=div(loc / UNIT, tp))
        per["hota"] = np.sqrt(per["deta"] * per["assa"])
    res = {n: float(v.mean()) for n, v in per.items()}
    res.update(hota_alpha=per["hota"], deta_alpha=per["deta"], assa_alpha=per["assa"], hota0=float(per["hota"][0]), loca0=float(per["loca"][0]))
    return res


# ------------------------------------------------------------------------------------------------ the published algorithm, float64
def hota_float(sims, cols, rows, G, P):
    """HOTA of one clip as published, in float64: ``sims`` [F] of [G, N] similarities (NaN: no pair), ``cols`` [F] of [N] (the
    predicted identity of j; -1 absent, -2 a detection without one: it can only be a false positive), ``rows`` [F] of row words.
    Returns (ints [19, 4] float64 (tp, fn, fp, loc in units of 2^-20), floats [19, 3], match [F, G])."""
    pot, rf, cf, extra = np.zeros((G, P)), np.zeros(G), np.zeros(P), 0
    for sim, col, row in zip(sims, cols, rows):
        ok = ~np.isnan(sim)
        s = np.where(ok, sim, 0.0)
        den = s.sum(1)[:, None] + s.sum(0)[None, :] - s
        n = np.where(ok & (den > 0), s / np.where(den > 0, den, 1.0), 0.0)
        for j in np.flatnonzero(np.asarray(col) >= 0):
            pot[:, col[j]] += n[:, j]
            cf[col[j]] += 1
        rf += [row >> g & 1 for g in range(G)]
        extra += int((np.asarray(col) == -2).sum())
    den = rf[:, None] + cf[None, :] - pot
    gas = np.where(den > 0, pot / np.where(den > 0, den, 1.0), 0.0)
    tp, loc, mc = np.zeros(ALPHAS), np.zeros(ALPHAS), np.zeros((ALPHAS, G, P))
    match = -np.ones((len(sims), G), np.int64)
    for r, (sim, col, _) in enumerate(zip(sims, cols, rows)):
        ok = ~np.isnan(sim)
        s = np.where(ok, sim, 0.0)
        score = np.where(ok, gas[:, np.maximum(col, 0)] * s, 0.0)
        for g, j in zip(*linear_sum_assignment(score, maximize=True)):
            if not ok[g, j]:
                continue
            match[r, g] = j
            for i in range(ALPHAS):
                if s[g, j] >= (i + 1) / 20.0:
                    tp[i] += 1
                    loc[i] += s[g, j] * UNIT
                    mc[i, g, col[j]] += 1
    den = rf[None, :, None] + cf[None, None, :] - mc
    with np.errstate(invalid="ignore", divide="ignore"):
        floats = np.stack([np.where(mc > 0, mc * mc / den, 0.0).sum((1, 2)), np.where(mc > 0, mc * mc / rf[None, :, None], 0.0).sum((1, 2)),
                           np.where(mc > 0, mc * mc / cf[None, None, :], 0.0).sum((1, 2))], 1)
    return np.stack([tp, rf.sum() - tp, cf.sum() + extra - tp, loc], 1), floats, match
