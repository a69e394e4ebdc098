"""-m gpu: the lane-track kernels (k_track_lane_start, k_track_lane_frame, through sqair_track_lane_test) against the float64
reference of tests/track_lane_ref.py on caller tensors: K in {1, 2, 5, 64, 65, 256} -- one particle, a wave, a wave boundary, the
whole workgroup --, F in {1, 3, 6} (lag * T with T in {1, 2}), N = 4 on the product library and N = 14 on the wide one, 50 x 50
frames and a 12 x 9 case whose boxes are larger than the frame.

The inputs are tests/track_lane_ref.make_paths' (genealogies that coalesce, paths that end fresh, ids that move between slots,
objects born inside the window, twins, a degenerate box, a best row whose newest frame is empty, the three non-finite lanes); the
comparison is tests/track_lane_check.py's, whose bars are tests/forecast_lane_check.py's at S = 1.  tests/test_track_lane_ref.py
holds these exact inputs against the 1 % cap on near-threshold decisions.  The worst observed margins (error / bar per field) are
recorded in profiles/track_lane_parity.json.

Last, the start kernel against the lane estimate (sqair_lane_estimate_test) on the rows of frame F - 1: the two share their device
functions, so weights, best row, the best row's words and the support are the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import track_lane_check as TC
from tests import track_lane_ref as TL
from tests.abi_host import open_handle

pytestmark = pytest.mark.gpu

_handles = {}


def _handle(wide, N, hw):
    key = (wide, N, hw)
    if key not in _handles:
        _handles[key] = open_handle(_capi.WIDE_LIB_PATH if wide else None, hw, k_particles=2, n_steps_per_image=N, n_what=6)
    return _handles[key]


def run(lib, h, g, F, K, N, iou_min, log_w=True, only=None):
    """The two kernels on the inputs ``g``; returns {name: array} of the outputs (``only``: the pointers bound besides best_row)."""
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()
    d = [dev(x) for x in (g.where, g.presence, g.obj_id)]
    valid = torch.as_tensor(np.ascontiguousarray(g.valid), dtype=torch.int32).cuda()
    lw = dev(g.log_w) if log_w else None
    shapes = _capi.track_lane_shapes(F, g.B, K, N)
    names = [n for n in shapes if only is None or n in only or n == "best_row"]
    o = {n: torch.full(shapes[n], -7, dtype=torch.int32 if n in _capi.TRACK_LANE_INT_FIELDS else torch.float32, device="cuda")
         for n in names}
    lane = _capi.SqairTraceLane(iou_min=iou_min, **{n: t.data_ptr() for n, t in o.items()})
    nb = lib.sqair_trace_lane_scratch_bytes(h, g.B, K)
    scratch = torch.zeros(nb // 4, dtype=torch.float32, device="cuda")
    s = torch.cuda.current_stream()
    rc = lib.sqair_track_lane_test(h, *[t.data_ptr() for t in d], valid.data_ptr(), None if lw is None else lw.data_ptr(), F, g.B, K,
                                   C.byref(lane), scratch.data_ptr(), nb, C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}


def measure(case):
    """One case: the device outputs checked against the reference; returns (margins, counts)."""
    K, F, N, wide, hw, iou_min = case
    lib, h = _handle(wide, N, hw)
    g = TL.make_paths(case)
    got = run(lib, h, g, F, K, N, iou_min)
    again = run(lib, h, g, F, K, N, iou_min)
    for n in got:   # a second call on the same inputs: identical bytes
        assert np.array_equal(got[n].view(np.uint32), again[n].view(np.uint32)), n
    ref = TL.lane_tracks(g.where, g.presence, g.obj_id, g.valid, g.log_w, K, hw, iou_min)
    assert ref.bad[-3:].all() and not ref.bad[:-3].any()
    margins, counts = TC.check(got, ref, g.where, g.presence, g.valid, K, hw, iou_min)
    # alive at the newest frame is the support: the same weights added in the same order
    assert np.array_equal(got["alive"][F - 1].view(np.uint32), got["support"].view(np.uint32))
    return margins, counts


@pytest.mark.parametrize("case", TL.CASES, ids=[TL.case_id(c) for c in TL.CASES])
def test_lane_track_kernels_against_fp64(case):
    K, F = case[:2]
    margins, counts = measure(case)
    print(TL.case_id(case), {k: "{:.3f}".format(v) for k, v in margins.items()}, counts)
    assert counts["decisions"] > 1 and counts["skipped"] <= 0.01 * counts["decisions"], counts
    assert counts["stats_checked"] > 0
    if K <= 8 and F > 1:
        assert counts["alive_zero"] > 0, counts     # an object no path holds at an older frame: NaN statistics were checked
    if K == 1:
        assert counts["std_zero"] == counts["stats_checked"]     # one path: box_std is exactly 0 in the reference, within A on the device


def test_optional_outputs_and_null_log_w():
    """Every pointer but best_row may be NULL, log_w NULL means uniform, and the outputs that are bound do not depend on the others."""
    case = (5, 6, 4, False, (50, 50), 0.5)
    K, F, N, wide, hw, iou_min = case
    lib, h = _handle(wide, N, hw)
    g = TL.make_paths(case)
    g.log_w = np.zeros_like(g.log_w)
    full = run(lib, h, g, F, K, N, iou_min)
    assert (full["weights"] == np.float32(1.0) / np.float32(K)).all()
    for only in ((), ("alive",), ("box_std", "count_prob"), ("support", "box0"), ("first_frame", "valid_mass")):
        part = run(lib, h, g, F, K, N, iou_min, log_w=False, only=only)
        for n in part:
            assert np.array_equal(part[n].view(np.uint32), full[n].view(np.uint32)), (only, n)


# ---- the start kernel and the lane estimate on the same rows -------------------------------------------------------------------
# k_lane_estimate (T = 1, lw zeros) and k_track_lane_start form the weights, the best row, its objects and the association of every
# particle from one set of device functions (csrc/sqair_lane.h).  The estimate knows no mask: it is given the rows of frame F - 1 as
# the trace's gather leaves them, zero where invalid -- for the start kernel the same rows, mask or no mask.  The support is a sum of
# the same weights over the same decisions in the same order, whatever the IoUs are: the same bits.
@pytest.mark.parametrize("case", [(1, 3, 4, False, (50, 50), 0.5), (5, 6, 4, False, (50, 50), 0.5), (65, 3, 4, False, (12, 9), 0.7),
                                  (256, 1, 4, False, (50, 50), 0.5)], ids=lambda c: TL.case_id(c))
def test_estimate_and_lane_tracks_agree_on_the_newest_frame(case):
    K, F, N, wide, hw, iou_min = case
    lib, h = _handle(wide, N, hw)
    g = TL.make_paths(case)
    B = g.B
    gone = g.valid == 0
    g.where[gone], g.presence[gone], g.obj_id[gone] = 0.0, 0.0, 0.0
    got = run(lib, h, g, F, K, N, iou_min, only=("weights", "presence", "obj_id", "box0", "support"))
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()
    d_where, d_pres, d_ids, d_lw0 = dev(g.where[F - 1]), dev(g.presence[F - 1]), dev(g.obj_id[F - 1]), dev(g.log_w)
    d_lw = dev(np.zeros((1, B * K), np.float32))
    z = lambda shp, dt=torch.float32: torch.full(shp, -7, dtype=dt, device="cuda")
    eo = dict(best_row=z((1, B), torch.int32), weights=z((1, B, K)), presence=z((1, B, N)), obj_id=z((1, B, N)), box=z((1, B, N, 4)),
              support=z((1, B, N)))
    est = _capi.SqairLaneEstimate(iou_min=iou_min, log_w=d_lw0.data_ptr(), **{n: t.data_ptr() for n, t in eo.items()})
    rc = lib.sqair_lane_estimate_test(h, d_where.data_ptr(), d_pres.data_ptr(), d_ids.data_ptr(), None, None, d_lw.data_ptr(), 1, B, K,
                                      C.byref(est), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    e = {n: t.cpu().numpy()[0] for n, t in eo.items()}
    bits = lambda x: np.ascontiguousarray(x).view(np.uint32)
    for n in ("weights", "best_row", "presence", "obj_id", "support"):
        assert np.array_equal(bits(e[n]), bits(got[n])), n
    assert float(np.abs(e["box"].astype(np.float64) - got["box0"]).max()) <= 16 * 2.0 ** -24 * max(hw)
    # the inputs did what they were built for: finite and non-finite lanes, objects, particles that do and that do not agree
    assert (e["best_row"][-3:] == -1).all() and (e["best_row"][:-3] >= 0).all() and np.isnan(e["support"][-3:]).all()
    assert (e["presence"] != 0).any() and np.isfinite(e["support"][:-3]).all()
    if K >= 5:
        assert ((e["support"][:-3] > 0) & (e["support"][:-3] < 1)).any()
