"""The comparison of a device lane estimate with the float64 reference (tests/estimate_ref.py), shared by the kernel test and the
stream test (no GPU import).

Tolerances.  Integer outputs and copied words are exact.  Weights, ess, count_prob, expected_count and support lie within the fp32
rounding band of the header's fixed-order sums (smc_ref.rounding_band for S; the same first-order bound, _sum_band, for the sums
of w_k), capped at 1e-5 relative as in the SMC test; below the smallest normal fp32 number, 2^-126, the format has no relative
precision left, so that much is allowed absolutely (a weight of e^-100 is 4e-44 in float64 and 0 or a subnormal on the device).
Boxes lie within 16 * 2^-24 * max(H, W) pixels: a NumPy fp32 restatement of the formula stays within 2 * 2^-24 * max(H, W) of
float64 on these inputs, the factor 8 covers the device's expf and tanhf.  A decision (does particle k agree on object j, with
which slot) is skipped and counted when the reference's best IoU lies within 1e-5 of iou_min (the fp32 IoU error of the same
restatement is below 2e-6), or when its two best IoUs lie within 1e-5 of each other and the best is not clearly below iou_min
(only then does the slot matter); map_count when the two largest count_prob lie within their bands.  At most 1 % of the decisions
may be skipped.  A skipped agreement widens the support's interval by that particle's weight.  box_mean is compared where no
decision of its (lane, object) was skipped: box_mean = sum w_k x_k / support, so its error is the boxes' own tolerance plus the
relative band of the two sums times the size of the coordinates, (max |x_k| + |box_mean|) (band / support + 2 u)."""
import numpy as np

from tests import estimate_ref as E
from tests import smc_ref as S

U = S.FP32_EPS
CAP = 1e-5
TINY = 2.0 ** -126
NEAR = 1e-5


def _sum_band(terms, term_err):
    """First-order fp32 bound on the error of sum_k terms[..., k] added in index order: the terms' own errors plus u |prefix| for
    every addition that is not exact in fp32 (smc_ref.rounding_band's bound for S, for any non-negative terms)."""
    t32 = terms.astype(np.float32).astype(np.float64)
    c = np.cumsum(t32, -1)
    prev = np.concatenate([np.zeros(c.shape[:-1] + (1,)), c[..., :-1]], -1)
    inexact = (prev.astype(np.float32) + t32.astype(np.float32)).astype(np.float64) != prev + t32
    return term_err.sum(-1) + U * np.where(inexact, np.abs(c), 0.0).sum(-1)


def _band_Q(w, K):
    """rounding_band for sum e_k^2 (tests/test_smc_kernel.py): a -> 2a and m -> 2m double e_k's subtraction term, as squaring does."""
    from types import SimpleNamespace
    return S.rounding_band(SimpleNamespace(a=2 * w.a, m=2 * w.m, e=w.e * w.e), K)


def _weight_err(w, K):
    """Per particle, the absolute fp32 error bound of w_k = e_k / S: e_k's own (the subtraction, expf), S's band, the division."""
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(w.a - w.m[:, None])
        rel = np.where((d == 0) | (w.e == 0), 0.0, U * d + S.ULP2) + (S.rounding_band(w, K) / w.S)[:, None] + U
        wk = w.e / w.S[:, None]
    return wk, np.minimum(rel, CAP) * wk + TINY / w.S[:, None]


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)



def new_counts():
    return dict(decisions=0, skipped=0, map_checked=0, map_skipped=0, box_mean_checked=0, agreeing=0, disagreeing=0)


def check(got, ref, where, pres, K, hw, iou_min, canvas=None, names=None, counts=None):
    """Asserts every output of ``got`` (name -> array, as SqairLaneEstimate names them) against ``ref`` = E.estimate(...) of the
    per-row inputs ``where`` [T, R, N, 4], ``pres`` [T, R, N] (``canvas`` [T, R, H, W] when mean_canvas is among the outputs).
    ``names``: the weight pattern of each lane, for the exact values of the "equal" and "dominant" ones.  Adds to ``counts`` (what
    was checked, what was skipped near a threshold) and returns it; the caller holds the skipped share against its cap."""
    T, R, N = pres.shape
    B = R // K
    with_canvas = canvas is not None
    counts = new_counts() if counts is None else counts
    names = [""] * B if names is None else names
    fin = ~ref.bad
    box_tol = 16 * U * max(hw)

    # ---- non-finite lanes: NaN numbers, -1 indices, zero objects
    for name in ("weights", "ess", "count_prob", "expected_count", "support", "box_mean") + (("mean_canvas",) if with_canvas else ()):
        assert np.isnan(got[name][~fin]).all(), name
        assert np.isfinite(got[name][fin]).all(), name
    assert (got["best_row"][~fin] == -1).all() and (got["map_count"][~fin] == -1).all()
    for name in ("presence", "obj_id", "where", "what", "box"):
        assert not _bits(got[name][~fin]).any(), name

    # ---- integer outputs and copied words: exact
    assert np.array_equal(got["best_row"], ref.best_row), np.argwhere(got["best_row"] != ref.best_row)[:4]
    for name in ("presence", "obj_id", "where", "what"):
        assert np.array_equal(_bits(got[name]), _bits(getattr(ref, name))), name
    err = np.abs(got["box"].astype(np.float64) - ref.box)
    print("box: worst error {:.3g} pixels, allowed {:.3g}".format(err.max(), box_tol))
    assert (err <= box_tol).all(), (err.max(), box_tol)
    assert not _bits(got["box"][ref.presence == 0]).any()

    for t in range(T):
        w = ref.w[t]
        f = fin[t]
        wk, w_err = _weight_err(w, K)
        # ---- weights and ESS
        e_w = np.abs(got["weights"][t].astype(np.float64) - wk)
        assert (e_w[f] <= w_err[f]).all(), [(names[b], e_w[b].max()) for b in np.flatnonzero(f & (e_w > w_err).any(1))[:4]]
        bS, bQ, Q = S.rounding_band(w, K), _band_Q(w, K), (w.e * w.e).sum(1)
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            tol_ess = np.minimum(2 * bS / w.S + bQ / Q + 4 * U + 2 * S.ULP2, CAP)
            e_ess = np.abs(got["ess"][t].astype(np.float64) - w.ess) / w.ess
        assert (e_ess[f] <= tol_ess[f]).all(), [(names[b], e_ess[b], tol_ess[b]) for b in np.flatnonzero(f & (e_ess > tol_ess))[:4]]
        if K == 1:
            assert (got["ess"][t][f] == 1.0).all() and (got["weights"][t][f] == 1.0).all()
        for b in np.flatnonzero(f):
            if names[b] == "equal":
                assert got["ess"][t, b] == K and (got["weights"][t, b] == np.float32(1.0) / np.float32(K)).all()
            if names[b] == "dominant":
                assert got["ess"][t, b] == 1.0 and got["weights"][t, b].max() == 1.0
        # ---- the count posterior
        n = (pres[t].reshape(B, K, N) != 0).sum(-1)
        cp_band = np.zeros((B, N + 1))
        for c in range(N + 1):
            sel = n == c
            cp = np.where(sel, wk, 0.0)
            band = np.minimum(_sum_band(cp, np.where(sel, w_err, 0.0)), CAP * cp.sum(-1) + K * TINY / w.S)
            e_c = np.abs(got["count_prob"][t, :, c].astype(np.float64) - ref.count_prob[t, :, c])
            assert (e_c[f] <= band[f]).all(), (c, [(names[b], e_c[b], band[b]) for b in np.flatnonzero(f & (e_c > band))[:4]])
            assert (got["count_prob"][t, :, c][f & ~sel.any(1)] == 0).all()     # no particle with that count: exactly 0
            cp_band[:, c] = band
        terms = wk * n
        band = np.minimum(_sum_band(terms, w_err * n + U * terms), CAP * terms.sum(-1) + K * N * TINY / w.S)
        e_n = np.abs(got["expected_count"][t].astype(np.float64) - ref.expected_count[t])
        assert (e_n[f] <= band[f]).all(), [(names[b], e_n[b], band[b]) for b in np.flatnonzero(f & (e_n > band))[:4]]
        for b in np.flatnonzero(f):
            order = np.argsort(-ref.count_prob[t, b], kind="stable")
            c0, c1 = order[0], order[1]
            if ref.count_prob[t, b, c0] - ref.count_prob[t, b, c1] <= cp_band[b, c0] + cp_band[b, c1]:
                counts["map_skipped"] += 1
                assert got["map_count"][t, b] in (c0, c1)
            else:
                counts["map_checked"] += 1
                assert got["map_count"][t, b] == ref.map_count[t, b], (names[b], got["map_count"][t, b], ref.count_prob[t, b])
        # ---- support and consensus box
        for b in np.flatnonzero(f):
            for j in range(N):
                if ref.presence[t, b, j] == 0:
                    assert got["support"][t, b, j] == 0 and not got["box_mean"][t, b, j].any()
                    continue
                best, second = ref.iou_best[t, b, :, j], ref.iou_second[t, b, :, j]
                has = best >= 0                                   # particles with a present slot: the others never agree
                near_thr = has & (np.abs(best - iou_min) <= NEAR)
                near_tie = has & (best - second <= NEAR) & (best >= iou_min - NEAR)
                counts["decisions"] += K
                counts["skipped"] += int((near_thr | near_tie).sum())
                agree = ref.agree[t, b, :, j]
                counts["agreeing"] += int(agree.sum())
                counts["disagreeing"] += int((has & ~agree).sum())
                sure = np.where(agree & ~near_thr, wk[b], 0.0)    # particles that agree whatever the rounding
                maybe = np.where(near_thr, wk[b], 0.0)
                band = min(_sum_band(sure + maybe, w_err[b] * ((sure + maybe) > 0)), CAP * (sure + maybe).sum() + K * TINY / w.S[b])
                sup = float(got["support"][t, b, j])
                assert sure.sum() - band <= sup <= sure.sum() + maybe.sum() + band, (names[b], j, sup, ref.support[t, b, j], band)
                assert sup >= wk[b, ref.best_row[t, b] % K] - band      # the best row agrees with itself
                if near_thr.any() or near_tie.any():
                    continue
                counts["box_mean_checked"] += 1
                x = E.boxes(where[t].reshape(B, K, N, 4)[b][np.arange(K), np.maximum(ref.match[t, b, :, j], 0)], hw)
                xmax = np.abs(x[agree]).max(0)
                bm = ref.box_mean[t, b, j]
                tol = box_tol + (xmax + np.abs(bm)) * (band / ref.support[t, b, j] + 2 * U)
                e_b = np.abs(got["box_mean"][t, b, j].astype(np.float64) - bm)
                assert (e_b <= tol).all(), (names[b], j, e_b, tol)
        # ---- the posterior mean reconstruction
        if with_canvas:
            # (a decoder's canvas may be negative: the sum's error is bounded through the sum of the terms' magnitudes, as for any
            #  fixed-order sum of terms of either sign; for a non-negative canvas that is the mean itself)
            cv = np.abs(canvas[t].reshape(B, K, -1).astype(np.float64))
            for b in np.flatnonzero(f):
                mean = ref.mean_canvas[t, b].reshape(-1)
                size = wk[b] @ cv[b]
                tol = np.minimum(w_err[b] @ cv[b] + U * (K + 1) * size, CAP * size + K * TINY / w.S[b])
                e_m = np.abs(got["mean_canvas"][t, b].reshape(-1).astype(np.float64) - mean)
                assert (e_m <= tol).all(), (names[b], e_m.max(), tol[np.argmax(e_m)])
    return counts
