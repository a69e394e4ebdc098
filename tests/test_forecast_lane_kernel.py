"""-m gpu: the lane-forecast kernels (k_forecast_lane_start, k_forecast_lane_frame, through sqair_forecast_lane_test) against the
float64 reference of tests/forecast_lane_ref.py on caller tensors: (K, S) in {(1, 1), (1, 8), (2, 3), (5, 4), (64, 1), (65, 3),
(256, 4)} -- one wave, a wave boundary, every thread of the workgroup, four rollouts per thread --, F in {1, 3}, N = 4 on the
product library and N = 14 on the wide one, 50 x 50 frames and a 12 x 9 case whose boxes are larger than the frame.

The inputs are tests/forecast_lane_ref.make_rollouts' (objects that die and stay dead, ids that move between slots, twins, a
degenerate box, a fresh best row, the three non-finite lanes); the comparison, its bars and the derivation of box_std's are
tests/forecast_lane_check.py's.  tests/test_forecast_lane_ref.py holds these exact inputs against the 1 % cap on near-threshold
decisions.  The worst observed margins (error / bar per field) are recorded in profiles/forecast_lane_parity.json.

Last, the lane forecast's start kernel against the lane estimate (sqair_lane_estimate_test) on the same rows: the two share their
device functions, so weights, best row, the best row's words and the support are the same bits (K in {1, 5, 65, 256}, B = 3, N = 4,
12 x 9, a NaN lane or an all -inf lane)."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import forecast_lane_check as FC
from tests import forecast_lane_ref as FL
from tests.abi_host import open_handle

pytestmark = pytest.mark.gpu

_handles = {}


def _handle(wide, N, hw):
    key = (wide, N, hw)
    if key not in _handles:
        _handles[key] = open_handle(_capi.WIDE_LIB_PATH if wide else None, hw, k_particles=2, n_steps_per_image=N, n_what=6)
    return _handles[key]


def run(lib, h, g, F, K, S, N, iou_min, log_w=True, only=None):
    """The two kernels on the inputs ``g``; returns {name: array} of the outputs (``only``: the pointers bound besides best_row)."""
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()
    d = [dev(x) for x in (g.start_where, g.start_presence, g.start_obj_id, g.where, g.presence, g.obj_id)]
    lw = dev(g.log_w) if log_w else None
    shapes = _capi.forecast_lane_shapes(F, g.B, K, N)
    names = [n for n in shapes if only is None or n in only or n == "best_row"]
    o = {n: torch.full(shapes[n], -7, dtype=torch.int32 if n in _capi.FORECAST_LANE_INT_FIELDS else torch.float32, device="cuda")
         for n in names}
    lane = _capi.SqairForecastLane(iou_min=iou_min, **{n: t.data_ptr() for n, t in o.items()})
    nb = lib.sqair_forecast_lane_scratch_bytes(h, g.B, K)
    scratch = torch.zeros(nb // 4, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    rc = lib.sqair_forecast_lane_test(h, *[t.data_ptr() for t in d], None if lw is None else lw.data_ptr(), F, g.B, K, S,
                                      C.byref(lane), scratch.data_ptr(), nb, C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}


def measure(case):
    """One case: the device outputs checked against the reference; returns (margins, counts)."""
    K, S, F, N, wide, hw, iou_min = case
    lib, h = _handle(wide, N, hw)
    g = FL.case_inputs(case)
    got = run(lib, h, g, F, K, S, N, iou_min)
    again = run(lib, h, g, F, K, S, N, iou_min)
    for n in got:   # a second call on the same inputs: identical bytes
        assert np.array_equal(got[n].view(np.uint32), again[n].view(np.uint32)), n
    ref = FL.lane_forecast(g.start_where, g.start_presence, g.start_obj_id, g.where, g.presence, g.obj_id, g.log_w, K, S, hw, iou_min)
    assert ref.bad[-3:].all() and not ref.bad[:-3].any()
    margins, counts = FC.check(got, ref, g.where, K, S, hw, iou_min)
    FC.check_counts(got, ref, g.presence, K, S, margins)
    return margins, counts


@pytest.mark.parametrize("case", FL.CASES, ids=[FL.case_id(c) for c in FL.CASES])
def test_lane_forecast_kernels_against_fp64(case):
    K, S, F = case[:3]
    margins, counts = measure(case)
    print(FL.case_id(case), {k: "{:.3f}".format(v) for k, v in margins.items()}, counts)
    assert counts["decisions"] > 0 and counts["skipped"] <= 0.01 * counts["decisions"], counts
    assert counts["stats_checked"] > 0
    if K * S <= 8 and F > 1:
        assert counts["alive_zero"] > 0, counts     # an object every rollout lost: NaN statistics were checked
    if K * S == 1:
        assert counts["std_zero"] == counts["stats_checked"]     # one rollout: box_std is exactly 0 in the reference, within A on the device


def test_optional_outputs_and_null_log_w():
    """Every pointer but best_row may be NULL, log_w NULL means uniform, and the outputs that are bound do not depend on the others."""
    case = (5, 4, 3, 4, False, (50, 50), 0.5)
    K, S, F, N, wide, hw, iou_min = case
    lib, h = _handle(wide, N, hw)
    g = FL.case_inputs(case)
    g.log_w = np.zeros_like(g.log_w)
    full = run(lib, h, g, F, K, S, N, iou_min)
    assert (full["weights"] == np.float32(1.0) / np.float32(K)).all()
    for only in ((), ("alive",), ("box_std", "count_prob"), ("support", "box0")):
        part = run(lib, h, g, F, K, S, N, iou_min, log_w=False, only=only)
        for n in part:
            assert np.array_equal(part[n].view(np.uint32), full[n].view(np.uint32)), (only, n)


# ---- the two entry points on the same rows ---------------------------------------------------------------------------------
# k_lane_estimate (T = 1, lw zeros) and k_forecast_lane_start (F = 1, S = 1) form the weights, the best row, its objects and the
# association of every particle from one set of device functions (csrc/sqair_lane.h): on the same rows their outputs are the same
# bits.  Every present box of a particle is a word-for-word copy of one of N mutually disjoint boxes (the only ones a best row
# holds) or lies in the other half of the frame, so every IoU is exactly 1 or 0 by the kernels' own rule and no decision is near
# the threshold.
AGREE_HW, AGREE_N, AGREE_B = (12, 9), 4, 3


def _agree_inputs(K, bad):
    """where [R, N, 4], presence, obj_id [R, N], log_w [R], the first maximal particle of lane 0 and the best particle of lane 1."""
    from tests import estimate_ref as E
    N, B = AGREE_N, AGREE_B
    rng = np.random.default_rng(77 + K)
    scale = lambda n: rng.uniform(-2.3, -2.0, size=(n, 2))                      # sigmoid: 0.09 .. 0.12 of the frame
    where = np.zeros((B, K, N, 4), np.float32)
    pres = np.zeros((B, K, N), np.float32)
    ids = rng.integers(0, 50, size=(B, K, N)).astype(np.float32)
    log_w = (rng.standard_normal((B, K)) * 2).astype(np.float32)
    k1, k2 = (0, 0) if K == 1 else sorted(rng.choice(K, 2, replace=False).tolist())
    log_w[0, [k1, k2]] = log_w[0].max() + np.float32(1.0)                       # lane 0: two particles share the maximum
    best = [k1, int(log_w[1].argmax()), 0]
    assert (log_w[1] == log_w[1].max()).sum() == 1
    if bad == "nan":
        log_w[2, K // 2] = np.nan
    else:
        log_w[2, :] = -np.inf
    for b in range(B):
        # the pool: N boxes stacked along y in the left part of the frame, and what else a particle may hold: boxes on the right
        pool = np.concatenate([scale(N), np.full((N, 1), np.arctanh(-0.7)), np.arctanh(-0.8 + 0.3 * np.arange(N))[:, None]], -1)
        pool = pool.astype(np.float32)
        pb = E.boxes(pool, AGREE_HW)
        order = np.argsort(pb[:, 0])
        assert (pb[order[1:], 0] - (pb[order[:-1], 0] + pb[order[:-1], 2]) > 0.05).all()      # disjoint in y, by a margin
        assert (pb[:, 1] + pb[:, 3]).max() < 4.0
        for k in range(K):
            right = np.concatenate([scale(N), np.arctanh(rng.uniform(0.5, 0.8, size=(N, 1))), rng.standard_normal((N, 1))], -1)
            assert E.boxes(right, AGREE_HW)[:, 1].min() > 4.5                                  # ... and those start beyond them in x
            copy = rng.uniform(size=N) < 0.6
            where[b, k] = np.where(copy[:, None], pool[rng.integers(0, N, size=N)], right.astype(np.float32))
            pres[b, k] = rng.uniform(size=N) < 0.7
        where[b, best[b]] = pool[rng.permutation(N)]                                          # the best row: distinct pool boxes
        pres[b, best[b]] = 1.0 if b == 0 else [1.0, 0.0, 1.0, 0.0]                            # lane 1: some of its slots absent
        where[b][pres[b] == 0.0] = rng.standard_normal(((pres[b] == 0.0).sum(), 4)) * 0.3     # absent slots: anything
    R = B * K
    return where.reshape(R, N, 4), pres.reshape(R, N), ids.reshape(R, N), log_w.reshape(R), k1, best[1]


@pytest.mark.parametrize("bad", ["nan", "neg_inf"])
@pytest.mark.parametrize("K", [1, 5, 65, 256])
def test_estimate_and_lane_forecast_agree_on_the_same_rows(K, bad):
    N, B, hw = AGREE_N, AGREE_B, AGREE_HW
    lib, h = _handle(False, N, hw)
    where, pres, ids, log_w, k1, k_lane1 = _agree_inputs(K, bad)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()
    d_where, d_pres, d_ids, d_lw0, d_lw = dev(where), dev(pres), dev(ids), dev(log_w), dev(np.zeros((1, B * K), np.float32))
    z = lambda shp, dt=torch.float32: torch.full(shp, -7, dtype=dt, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    eo = dict(best_row=z((1, B), torch.int32), weights=z((1, B, K)), presence=z((1, B, N)), obj_id=z((1, B, N)), box=z((1, B, N, 4)),
              support=z((1, B, N)))
    est = _capi.SqairLaneEstimate(iou_min=0.5, log_w=d_lw0.data_ptr(), **{n: t.data_ptr() for n, t in eo.items()})
    rc = lib.sqair_lane_estimate_test(h, d_where.data_ptr(), d_pres.data_ptr(), d_ids.data_ptr(), None, None, d_lw.data_ptr(), 1, B, K,
                                      C.byref(est), s)
    assert rc == 0, lib.sqair_last_error(h)
    shapes = _capi.forecast_lane_shapes(1, B, K, N)
    fo = {n: z(shapes[n], torch.int32 if n in _capi.FORECAST_LANE_INT_FIELDS else torch.float32)
          for n in ("best_row", "weights", "presence", "obj_id", "box0", "support")}
    lane = _capi.SqairForecastLane(iou_min=0.5, **{n: t.data_ptr() for n, t in fo.items()})
    nb = lib.sqair_forecast_lane_scratch_bytes(h, B, K)
    scratch = torch.zeros(nb // 4, dtype=torch.float32, device="cuda")
    rc = lib.sqair_forecast_lane_test(h, d_where.data_ptr(), d_pres.data_ptr(), d_ids.data_ptr(), d_where.data_ptr(), d_pres.data_ptr(),
                                      d_ids.data_ptr(), d_lw0.data_ptr(), 1, B, K, 1, C.byref(lane), scratch.data_ptr(), nb, s)
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    e = {n: t.cpu().numpy()[0] for n, t in eo.items()}
    f = {n: t.cpu().numpy() for n, t in fo.items()}
    bits = lambda x: x.view(np.uint32)
    box_bits = np.array_equal(bits(e["box"]), bits(f["box0"]))
    box_err = float(np.abs(e["box"].astype(np.float64) - f["box0"]).max())
    print("K", K, bad, "box bit-equal:", box_bits, "max |box - box0|", box_err)
    for n in ("weights", "best_row", "presence", "obj_id", "support"):
        assert np.array_equal(bits(e[n]), bits(f[n])), n
    assert box_err <= 16 * 2.0 ** -24 * max(hw)
    # the inputs did what they were built for: the first of the two maxima, a best row with absent slots, a non-finite lane
    assert e["best_row"].tolist() == [k1, K + k_lane1, -1]
    assert (e["presence"][0] != 0).all() and (e["presence"][1] != 0).tolist() == [True, False, True, False]
    assert np.isnan(e["weights"][2]).all() and np.isnan(e["support"][2]).all() and not e["presence"][2].any()
    assert np.isfinite(e["support"][:2]).all() and (e["support"][0] > 0).all()
    if K >= 5:
        assert ((e["support"][:2] > 0) & (e["support"][:2] < 1)).any()     # particles that do and particles that do not agree
