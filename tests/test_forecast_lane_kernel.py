"""-m gpu: the lane-forecast kernels (k_forecast_lane_start, k_forecast_lane_frame, through sqair_forecast_lane_test) against the
float64 reference of tests/forecast_lane_ref.py on caller tensors: (K, S) in {(1, 1), (1, 8), (2, 3), (5, 4), (64, 1), (65, 3),
(256, 4)} -- one wave, a wave boundary, every thread of the workgroup, four rollouts per thread --, F in {1, 3}, N = 4 on the
product library and N = 14 on the wide one, 50 x 50 frames and a 12 x 9 case whose boxes are larger than the frame.

The inputs are tests/forecast_lane_ref.make_rollouts' (objects that die and stay dead, ids that move between slots, twins, a
degenerate box, a fresh best row, the three non-finite lanes); the comparison, its bars and the derivation of box_std's are
tests/forecast_lane_check.py's.  tests/test_forecast_lane_ref.py holds these exact inputs against the 1 % cap on near-threshold
decisions.  The worst observed margins (error / bar per field) are recorded in profiles/forecast_lane_parity.json."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from tests import forecast_lane_check as FC
from tests import forecast_lane_ref as FL

pytestmark = pytest.mark.gpu

_handles = {}


def _handle(wide, N, hw):
    key = (wide, N, hw)
    if key not in _handles:
        lib = _capi.lib(_capi.WIDE_LIB_PATH if wide else None)
        cfg = make_config(make_flags(k_particles=2, n_steps_per_image=N, n_what=6), hw)
        h = C.c_void_p()
        assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
        _handles[key] = (lib, h)
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
