"""The comparison of a device lane forecast with the float64 reference (tests/forecast_lane_ref.py), shared by the kernel test and
the whole-forecast test (no GPU import).  The bars are tests/estimate_check.py's, restated for n = K * S rollouts:

* integer outputs and copied words are exact;
* weights within ``estimate_check._weight_err``; a rollout's weight w_q = fl(w_k / S) carries that error / S plus one rounding;
* sums of weights (support, alive, count_prob) within the fp32 rounding band of the fixed-order sum over their n terms
  (``estimate_check._sum_band``), capped at 1e-5 relative;
* box0 within 16 * 2^-24 * max(H, W) pixels; box_mean within that plus the relative band of its two sums times the size of the
  coordinates, as the estimate's box_mean;
* association decisions within 1e-5 of the threshold (or of a tie) are skipped and counted: the objects they touch get the interval
  check of the estimate's support for ``support`` and are left out of the per-frame statistics.

box_std, derived here.  With weights p_q = w_q / alive (they sum to 1), std = || x - mean ||_p, a weighted L2 norm.  The device forms
d'_q = fl(x'_q - mean') from boxes x' = x + eps (|eps| <= t_box, the box bar) and its own mean' = mean + dm (|dm| <= t_mean, the
box_mean bar), so d' = d + eta with |eta_q| <= t_box + t_mean + u |d_q|, and by the triangle inequality of the norm
| ||d'||_p - ||d||_p | <= max_q |eta_q| =: A -- an ABSOLUTE bar in pixels that holds at std = 0, where a relative one says nothing.  (The
exact identity sum p (x - mean')^2 = var + dm^2 is inside it: sqrt(var + dm^2) - std <= |dm|.)  The rest is relative: the n squares,
products and additions of non-negative terms ((n + 3) u on the variance, first order), the weights and alive in the quotient
(2 band / alive), halved by the square root, plus the root's and the division's own roundings:
    tol_std = A + (std + A) (band / alive + ((n + 3) / 2 + 2) u),   A = t_box + t_mean + u max_q |x_q - mean|.
"""
import numpy as np

from tests import estimate_check as EC
from tests import estimate_ref as E
from tests import forecast_lane_ref as FL

U, CAP, TINY, NEAR = EC.U, EC.CAP, EC.TINY, EC.NEAR
NAN_FIELDS = ("weights", "support", "alive", "box_mean", "box_std", "count_prob")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _margin(m, name, err, tol):
    """Records the worst err / tol of a field (1 = at the bar) and returns whether every entry is inside."""
    err, tol = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(tol, dtype=np.float64))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(err == 0, 0.0, err / tol)
    if ratio.size:
        m[name] = max(m.get(name, 0.0), float(ratio.max()))
    return bool((err <= tol).all())


def check(got, ref, rollout_where, K, S, hw, iou_min, margins=None, counts=None):
    """Asserts every output of ``got`` (name -> array, as SqairForecastLane names them) against ``ref`` = FL.lane_forecast(...);
    ``rollout_where`` [F, R*S, N, 4].  Adds the worst err / tol per field to ``margins`` and what was checked / skipped to
    ``counts``; returns (margins, counts)."""
    margins = {} if margins is None else margins
    counts = dict(decisions=0, skipped=0, stats_checked=0, std_zero=0, alive_zero=0, died=0) if counts is None else counts
    F, B, N = ref.alive.shape
    KS = K * S
    fin = ~ref.bad
    box_tol = 16 * U * max(hw)
    kq = np.arange(KS) // S
    # ---- non-finite lanes: NaN numbers, best_row -1, no objects
    for name in NAN_FIELDS:
        g = got[name]
        lane_axis = 0 if name in ("weights", "support") else 1
        assert np.isnan(np.compress(~fin, g, lane_axis)).all(), name
    assert (got["best_row"][~fin] == -1).all()
    for name in ("presence", "obj_id", "box0"):
        assert not _bits(got[name][~fin]).any(), name
    # ---- integer outputs and copied words: exact
    assert np.array_equal(got["best_row"], ref.best_row), np.argwhere(got["best_row"] != ref.best_row)[:4]
    for name in ("start_where", "start_presence", "start_obj_id", "presence", "obj_id"):
        assert np.array_equal(_bits(got[name]), _bits(getattr(ref, name))), name
    assert _margin(margins, "box0", np.abs(got["box0"].astype(np.float64) - ref.box0), box_tol), margins
    assert not _bits(got["box0"][ref.presence == 0]).any()
    # ---- weights
    wk, w_err = EC._weight_err(ref.w, K)
    assert _margin(margins, "weights", np.abs(got["weights"].astype(np.float64) - wk)[fin], w_err[fin]), margins
    if K == 1:
        assert (got["weights"][fin] == 1.0).all()
    decisions, skip = FL.near_threshold(ref, iou_min, NEAR)
    counts["decisions"] += decisions
    counts["skipped"] += int(skip.sum())
    box_r = E.boxes(rollout_where, hw).reshape(F, B, KS, N, 4)
    for b in np.flatnonzero(fin):
        wq = wk[b][kq] / S
        wq_err = w_err[b][kq] / S + U * wq
        lim = lambda terms, terr: min(EC._sum_band(terms, terr), CAP * terms.sum() + KS * TINY / ref.w.S[b])
        # ---- support, alive and the box statistics
        for j in range(N):
            if ref.presence[b, j] == 0:   # an absent best-row slot: zeros
                assert got["support"][b, j] == 0 and not got["alive"][:, b, j].any()
                assert not got["box_mean"][:, b, j].any() and not got["box_std"][:, b, j].any()
                continue
            agree, near = ref.agree[b, :, j], skip[b, :, j]
            sure, maybe = np.where(agree & ~near, wk[b], 0.0), np.where(near, wk[b], 0.0)
            band = min(EC._sum_band(sure + maybe, w_err[b] * ((sure + maybe) > 0)), CAP * (sure + maybe).sum() + K * TINY / ref.w.S[b])
            sup = float(got["support"][b, j])
            assert sure.sum() - band <= sup <= sure.sum() + maybe.sum() + band, (b, j, sup, ref.support[b, j], band)
            assert sup >= wk[b, ref.best_row[b] % K] - band       # the best row is associated with itself
            if not near.any():
                _margin(margins, "support", abs(sup - ref.support[b, j]), band)
            if near.any():
                continue
            prev = np.inf
            for f in range(F):
                hit = ref.hit[f, b, :, j]
                terms = np.where(hit, wq, 0.0)
                band = lim(terms, np.where(hit, wq_err, 0.0))
                al, al_ref = float(got["alive"][f, b, j]), ref.alive[f, b, j]
                assert _margin(margins, "alive", abs(al - al_ref), band), (b, j, f, al, al_ref, band)
                assert al <= sup + band and al <= prev + band     # unnormalised, <= support, non-increasing in f
                prev = al
                gm, gs = got["box_mean"][f, b, j].astype(np.float64), got["box_std"][f, b, j].astype(np.float64)
                if not hit.any():                                 # nothing to average: NaN, and alive exactly 0
                    counts["alive_zero"] += 1
                    assert al == 0 and np.isnan(gm).all() and np.isnan(gs).all(), (b, j, f, al, gm, gs)
                    continue
                if al_ref < 2.0 ** -100:                          # below fp32's normal range after the division by S and alive: the
                    counts["underflow"] = counts.get("underflow", 0) + 1   # format has no relative precision left (estimate_check: TINY)
                    continue
                x = box_r[f, b][np.arange(KS), np.maximum(ref.slot[f, b, :, j], 0)][hit]        # [n_hit, 4]
                bm, bs = ref.box_mean[f, b, j], ref.box_std[f, b, j]
                t_mean = box_tol + (np.abs(x).max(0) + np.abs(bm)) * (band / al_ref + 2 * U)
                assert _margin(margins, "box_mean", np.abs(gm - bm), t_mean), (b, j, f, gm, bm, t_mean)
                A = box_tol + t_mean + U * np.abs(x - bm).max(0)
                t_std = A + (bs + A) * (band / al_ref + ((KS + 3) / 2 + 2) * U)
                assert _margin(margins, "box_std", np.abs(gs - bs), t_std), (b, j, f, gs, bs, t_std)
                counts["stats_checked"] += 1
                counts["std_zero"] += int((bs == 0).all())
            counts["died"] += int((ref.hit[0, b, :, j].sum() > ref.hit[F - 1, b, :, j].sum()) or
                                  (ref.agree[b, :, j].sum() * S > ref.hit[0, b, :, j].sum()))
    return margins, counts


def check_counts(got, ref, rollout_presence, K, S, margins):
    """count_prob against the reference: per (f, b, c) the fp32 band of the fixed-order sum of the weights of the rollouts that hold c
    objects; exactly 0 where no rollout holds c; each row sums to 1 within the bands."""
    F, B, N = ref.alive.shape
    KS = K * S
    kq = np.arange(KS) // S
    wk, w_err = EC._weight_err(ref.w, K)
    n = (rollout_presence != 0).reshape(F, B, KS, N).sum(-1)
    for b in np.flatnonzero(~ref.bad):
        wq = wk[b][kq] / S
        wq_err = w_err[b][kq] / S + U * wq
        for f in range(F):
            total = 0.0
            for c in range(N + 1):
                sel = n[f, b] == c
                terms = np.where(sel, wq, 0.0)
                band = min(EC._sum_band(terms, np.where(sel, wq_err, 0.0)), CAP * terms.sum() + KS * TINY / ref.w.S[b])
                g = float(got["count_prob"][f, b, c])
                assert _margin(margins, "count_prob", abs(g - ref.count_prob[f, b, c]), band), (b, f, c, g, ref.count_prob[f, b, c], band)
                if not sel.any():
                    assert g == 0
                total += band
            assert abs(float(got["count_prob"][f, b].astype(np.float64).sum()) - 1.0) <= total + (N + 1) * U
    return margins
