"""The comparison of device lane tracks with the float64 reference (tests/track_lane_ref.py), shared by the kernel test and the
stream test (no GPU import).  No bar of its own: everything the tracks share with the lane forecast -- weights, best row, copied
words, box0, support, and per frame alive, box_mean and box_std -- goes through tests/forecast_lane_check.check at S = 1, in the
forecast's frame order (newest frame first: there an object "dies" where, in the tracks' order, it is born); count_prob and
valid_mass get forecast_lane_check.check_counts' band, the fp32 band of the fixed-order sum of the weights that enter, without its
"sums to 1" (the tracks' count_prob sums to valid_mass); first_frame is an integer and exact."""
import numpy as np

from tests import estimate_check as EC
from tests import forecast_lane_check as FC

U, CAP, TINY, NEAR = FC.U, FC.CAP, FC.TINY, FC.NEAR
PER_FRAME = ("alive", "box_mean", "box_std", "count_prob")


def check(got, ref, where, presence, valid, K, hw, iou_min, margins=None, counts=None):
    """Asserts every output of ``got`` (name -> array, as SqairTraceLane names them, frames oldest -> newest) against ``ref`` =
    track_lane_ref.lane_tracks(...) of the traced rows ``where`` [F, R, N, 4], ``presence`` [F, R, N], ``valid`` [F, R].  Returns
    (margins, counts) as forecast_lane_check.check does."""
    margins = {} if margins is None else margins
    F, B, N = ref.alive.shape
    fwd = dict(got)
    for name in PER_FRAME:
        fwd[name] = got[name][::-1]
    for name in ("start_where", "start_presence", "start_obj_id"):   # (the tracks have no such outputs: nothing to compare)
        fwd[name] = getattr(ref.fwd, name)
    margins, counts = FC.check(fwd, ref.fwd, np.asarray(where)[::-1], K, 1, hw, iou_min, margins, counts)
    # ---- first_frame: exact; -1 exactly where the object is absent
    assert np.array_equal(got["first_frame"], ref.first_frame), np.argwhere(got["first_frame"] != ref.first_frame)[:4]
    assert np.array_equal(got["first_frame"] < 0, ref.presence == 0)
    # ---- count_prob and valid_mass: unnormalised sums of the weights of the valid rows
    fin = ~ref.bad
    assert np.isnan(got["valid_mass"][:, ~fin]).all() and np.isfinite(got["valid_mass"][:, fin]).all()
    wk, w_err = EC._weight_err(ref.w, K)
    ok = (np.asarray(valid) != 0).reshape(F, B, K)
    n = ((np.asarray(presence) != 0).reshape(F, B, K, N) & ok[..., None]).sum(-1)
    for b in np.flatnonzero(fin):
        lim = lambda terms, terr: min(EC._sum_band(terms, terr), CAP * terms.sum() + K * TINY / ref.w.S[b])
        for f in range(F):
            total = 0.0
            for c in range(N + 1):
                sel = ok[f, b] & (n[f, b] == c)
                band = lim(np.where(sel, wk[b], 0.0), np.where(sel, w_err[b], 0.0))
                g = float(got["count_prob"][f, b, c])
                assert FC._margin(margins, "count_prob", abs(g - ref.count_prob[f, b, c]), band), (b, f, c, g, ref.count_prob[f, b, c], band)
                if not sel.any():
                    assert g == 0
                total += band
            vm = float(got["valid_mass"][f, b])
            band = lim(np.where(ok[f, b], wk[b], 0.0), np.where(ok[f, b], w_err[b], 0.0))
            assert FC._margin(margins, "valid_mass", abs(vm - ref.valid_mass[f, b]), band), (b, f, vm, ref.valid_mass[f, b], band)
            if not ok[f, b].any():
                assert vm == 0
            # count_prob sums to valid_mass, not to 1
            assert abs(float(got["count_prob"][f, b].astype(np.float64).sum()) - vm) <= total + band + (N + 1) * U, (b, f)
    return margins, counts
