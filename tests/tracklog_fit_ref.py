"""The reference of motion calibration (include/sqair_hip.h: sqair_lane_tracklog_fit, the track log fit paragraph), restated from the
header and not from the kernel.  NumPy; the walk is a plain loop over (lane, column, axis, frame), every candidate of the grid at once
as a [Q, R] array.

``fit`` is points 1 to 5 in float64 -- only the box words and the scalars are fp32 values -- on ``tracklog_ref.smooth``'s ``state`` and
the slots of its columns (``slots``), with the filter's statements of tests/tracklog_ref.py (``start``, ``predict``, ``update``), not a
copy of them.  Beside every float64 term stands the fp32 RESTATEMENT: numpy ``float32``, the header's operations in the header's
order, ``motion_ref._fma`` where the header says ``fmaf``, and ``np.log`` of the float64-cast fp32 ``S``.  What a term of the restatement
differs by from float64 is the measured fp32 error of that term (``Fit.term_err``: per kind of term and per grid node [Q, R], the
worst of the case over lanes, columns, axes and frames); a sum's bar is four times that times the sum's number of terms (``bars``)
-- the project's rule, as tests/tracklog_score_ref.py argues it: the kernel adds fp32 terms in fp64, so the sum's error is the terms'
errors added.  The worst is taken PER NODE, not over the whole grid: a term's error grows with the term -- y comes out of a
cancellation and is divided by S, so at a node whose S is a hundredth of the data's the terms and their errors are a hundred times
larger -- and one bar for the grid would hold the nodes near the fit, where the terms are of order 1, to the error of the absurd
ones (on the recovery case 2e-2 a term against 1e-5).  A node's own worst is the tighter bar at every node.  Whether a term counts (S > 0, nis finite) is
decided in float64; ``Fit.undecided`` counts the terms the restatement decides otherwise, and the cases assert there is none."""
import collections

import numpy as np

from tests import tracklog_ref as R
from tests.motion_ref import _fma

COUNTS = ("n", "n_gap", "skipped")
SUMS = ("nis_sum", "lns_sum", "gap_nis_sum", "gap_lns_sum")
TERM_OF = dict(nis_sum="nis", lns_sum="lns", gap_nis_sum="nis", gap_lns_sum="lns")     # the kind of term each sum adds
N_OF = dict(nis_sum="n", lns_sum="n", gap_nis_sum="n_gap", gap_lns_sum="n_gap")       # the counter that is its number of terms

Fit = collections.namedtuple("Fit", "counts sums sums32 innov innov32 term_err innov_err undecided")


def slots(log, solve, lag):
    """The slot of every (frame, column) [lag, B, C] of a ``tracklog_ref.smooth`` result: point 2's smallest j of the column's id in a
    frame that counts, else -1 -- what the solve leaves in ``work``."""
    B, C = solve.track_id.shape
    out = -np.ones((lag, B, C), np.int64)
    for b in range(B):
        _, rec, counts = R.window(log, b, lag)
        for f in range(lag):
            if not counts[f]:
                continue
            for c in range(C):
                hit = np.flatnonzero(log["log_id"][b, rec[f]] == solve.track_id[b, c]) if solve.track_id[b, c] >= 0 else ()
                if len(hit):
                    out[f, b, c] = hit[0]
    return out


def grids(q_grid, r_grid):
    """The grids as the fp32 values the call is handed, float64 arrays broadcasting to [Q, R]."""
    return np.asarray(q_grid, np.float32).astype(np.float64)[:, None], np.asarray(r_grid, np.float32).astype(np.float64)[None, :]


def fit(log, frame_index, state, slot, q_grid, r_grid, v0_var, burn):
    """Points 1 to 5 on a log {name: array}, the solve's ``frame_index`` [lag, B] and ``state`` [lag, B, C] and the slots [lag, B, C]."""
    if len(q_grid) * len(r_grid) == 1:   # (tracklog_ref's statements take a one-element array for a scalar: walk the node twice)
        got = fit(log, frame_index, state, slot, tuple(q_grid) * 2, r_grid, v0_var, burn)
        return got._replace(counts=got.counts[:, :1], sums=got.sums[:, :1], sums32=got.sums32[:, :1], undecided=got.undecided // 2,
                            term_err={n: e[:1] for n, e in got.term_err.items()})
    qg, rg = grids(q_grid, r_grid)
    Q, Rn = qg.shape[0], rg.shape[1]
    qg, rg = np.broadcast_to(qg, (Q, Rn)), np.broadcast_to(rg, (Q, Rn))   # (no one-element arrays: see above)
    v0_var = float(np.float32(v0_var))
    lag, B, C = state.shape
    L = log["log_valid"].shape[1]
    counts, sums, sums32 = np.zeros((B, Q, Rn, 3), np.int64), np.zeros((B, Q, Rn, 4)), np.zeros((B, Q, Rn, 4))
    innov, innov32 = np.zeros((lag, B, C, 2, 2)), np.zeros((lag, B, C, 2, 2), np.float32)
    term_err, innov_err, undecided = dict(nis=np.zeros((Q, Rn)), lns=np.zeros((Q, Rn))), 0.0, 0
    zero = np.zeros((Q, Rn))
    with np.errstate(all="ignore"):
        for b in range(B):
            for c in range(C):
                for ax in range(2):
                    k = {np.float64: None, np.float32: None}
                    i, gap = 0, False
                    part, part32, cnt = np.zeros((4, Q, Rn)), np.zeros((4, Q, Rn)), np.zeros((3, Q, Rn), np.int64)
                    for f in range(lag):
                        st = state[f, b, c]
                        if st in (R.OUTSIDE, R.INVALID):                                                              # 1
                            continue
                        if st == R.GAP:                                                                               # 3
                            for ft in k:
                                k[ft] = R.predict(k[ft], qg.astype(ft), rg.astype(ft), ft)[0]
                            gap = True
                            continue
                        bx = log["log_box"][b, int(frame_index[f, b] % L), slot[f, b, c]]
                        z = {np.float64: 0.5 * np.float64(bx[2 + ax]) + np.float64(bx[ax]), np.float32: _fma(np.float32(0.5), bx[2 + ax], bx[ax])}
                        if k[np.float64] is None:                                                                     # 2
                            for ft in k:
                                k[ft] = R.start(z[ft], rg.astype(ft), v0_var, ft)
                            i, gap = 0, False
                            continue
                        term = {}                                                                                     # 4
                        for ft in k:
                            k[ft], S = R.predict(k[ft], qg.astype(ft), rg.astype(ft), ft)
                            y = (z[ft] - k[ft][0]) + zero.astype(ft)
                            nis = (y * y) / S
                            ok = (S > 0) & np.isfinite(nis)
                            safe = np.where(ok, S, 1).astype(np.float64)
                            term[ft] = y, S, np.where(ok, nis, 0).astype(np.float64), np.where(ok, np.log(safe), 0.0), ok
                            k[ft] = R.update(k[ft], S, z[ft], ft)
                        i += 1
                        (y, S, nis, lns, ok), (y32, S32, nis32, lns32, ok32) = term[np.float64], term[np.float32]
                        innov[f, b, c, ax], innov32[f, b, c, ax] = (y[0, 0], S[0, 0]), (y32[0, 0], S32[0, 0])
                        both = [v for v in (abs(float(y32[0, 0]) - y[0, 0]), abs(float(S32[0, 0]) - S[0, 0])) if np.isfinite(v)]
                        innov_err = max([innov_err] + both)
                        if i > burn:
                            undecided += int((ok != ok32).sum())
                            agree = ok & ok32
                            term_err["nis"] = np.maximum(term_err["nis"], np.where(agree, np.abs(nis32 - nis), 0.0))
                            term_err["lns"] = np.maximum(term_err["lns"], np.where(agree, np.abs(lns32 - lns), 0.0))
                            g = ok & gap
                            cnt += np.stack([ok, g, ~ok]).astype(np.int64)
                            part += np.stack([nis, lns, nis * g, lns * g])
                            part32 += np.stack([nis32 * ok, lns32 * ok, nis32 * g, lns32 * g])
                        gap = False
                    counts[b] += np.moveaxis(cnt, 0, -1)           # the partial sums of (c, a), added in (c, a) index order
                    sums[b] += np.moveaxis(part, 0, -1)
                    sums32[b] += np.moveaxis(part32, 0, -1)
    return Fit(counts, sums, sums32, innov, innov32, term_err, innov_err, undecided)


def bars(ref):
    """The bars of ``sums`` [B, Q, R, 4]: four times the case's worst error of a term of that kind at the node times the sum's number
    of terms."""
    n = {name: ref.counts[..., i] for i, name in enumerate(COUNTS)}
    return np.stack([4.0 * ref.term_err[TERM_OF[s]][None] * n[N_OF[s]] for s in SUMS], -1)


def nll_bars(ref):
    """[Q, R]: the bar of the pooled negative log-likelihood of every node, half the bars of lns_sum and nis_sum added over the lanes."""
    b = bars(ref).sum(0)
    return 0.5 * (b[..., SUMS.index("nis_sum")] + b[..., SUMS.index("lns_sum")])


def worst(term_err):
    """{kind: the largest term error over the grid}, for a report."""
    return {n: float(e.max()) for n, e in term_err.items()}


def nll(counts, sums):
    """1/2 (n ln 2 pi + lns_sum + nis_sum) of every node, pooled over the leading axis."""
    c, s = counts.sum(0), sums.sum(0)
    return 0.5 * (c[..., 0] * np.log(2.0 * np.pi) + s[..., 1] + s[..., 0])


def expected_terms(state, burn):
    """[B]: the innovations past ``burn`` of a lane, counted from ``state`` alone -- per column the sightings behind the first, less
    ``burn``, times the two axes."""
    seen = (state == R.SEEN).sum(0)                                  # [B, C]
    return 2 * np.maximum(seen - 1 - burn, 0).sum(1)


# ---- an independent derivation: the same likelihood from the dense Gaussian the model defines ------------------------------------------
def dense_nll(zs, q, r, v0_var):
    """-log p(z_1 .. z_m | z_0) of one axis of one track over consecutive stepped frames, ``zs`` its measurements (None in a gap;
    zs[0] the first sighting, which the walk conditions on): the model of the motion paragraph written out as one Gaussian.  The
    state at the first sighting is x_0 ~ N((z_0, 0), diag(r, v0_var)), x_{k+1} = F x_k + g a_k with F = [[1, 1], [0, 1]], g = (1/2, 1)
    and a_k ~ N(0, q), z_k = p_k + e_k with e_k ~ N(0, r): the later sightings are jointly Gaussian with mean H F^k (z_0, 0) and a
    covariance assembled here entry by entry; the density is evaluated with numpy.linalg (slogdet, solve).  No recursion."""
    F, g = np.array([[1.0, 1.0], [0.0, 1.0]]), np.array([0.5, 1.0])
    n = len(zs)
    Fk = [np.linalg.matrix_power(F, k) for k in range(n)]
    P0, Qm = np.diag([r, v0_var]), q * np.outer(g, g)
    cov_x = [[None] * n for _ in range(n)]                           # Cov(x_j, x_k) = F^j P0 F^kT + sum_{i < min(j, k)} F^(j-1-i) Q F^(k-1-i)T
    for j in range(n):
        for k in range(n):
            m = Fk[j] @ P0 @ Fk[k].T
            for i in range(min(j, k)):
                m = m + Fk[j - 1 - i] @ Qm @ Fk[k - 1 - i].T
            cov_x[j][k] = m
    seen = [k for k in range(1, n) if zs[k] is not None]
    if not seen:
        return 0.0, 0
    S = np.array([[cov_x[j][k][0, 0] + (r if j == k else 0.0) for k in seen] for j in seen])
    mean = np.array([(Fk[k] @ np.array([zs[0], 0.0]))[0] for k in seen])
    d = np.array([zs[k] for k in seen]) - mean
    return 0.5 * (len(seen) * np.log(2.0 * np.pi) + np.linalg.slogdet(S)[1] + d @ np.linalg.solve(S, d)), len(seen)
