"""-m gpu: the scoring kernel (k_lane_score, through sqair_lane_score_test) against the float64 reference of tests/score_ref.py, on
caller buffers, for the cases of tests/score_cases.py: 210 lanes, T = 6, (G, N) = (4, 4), (1, 4) and (16, 14) on the wide library --
every thread of the workgroup fills an entry of the IoU table there --, iou_min 0.5 and 0.3.

The integer outputs (``truth_match``, ``tp``, ``fn``, ``fp``, ``idsw``), ``counts`` and ``last_id`` are compared exactly;
``match_iou`` within four times the error of an fp32 NumPy restatement of sq_box_iou against float64, measured on these very inputs
(tests/score_ref.py: iou32_error; the factor covers the device's division; tests/test_score_ref.py keeps that tolerance below 1e-5
and prints it); ``iou_sum`` within that band times the lane's ``tp``.  A lane is left out from its first fragile frame on
(tests/score_ref.py: fragile_from), at most 1 % of the lanes -- tests/test_score_ref.py holds the same inputs to that cap from the
reference alone.  Also here: two passes of three frames give the bits of one pass of six (the accumulators and the memory are
handed on in place), and the per-frame outputs are optional.  With SQAIR_PARITY_DIR set the measured figures are written to
score_parity.json there (the copy under profiles/ is such a file); without it nothing is written."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import score_cases as SC
from tests import score_ref as R
from tests.abi_host import open_handle
from tests.kernel_unit import merge_parity

pytestmark = pytest.mark.gpu

INT_OUT = ("truth_match", "tp", "fn", "fp", "idsw")
NOTE = ("per case of tests/test_score_kernel.py: the largest error of match_iou against the float64 reference and what is "
        "allowed (four times the measured error of an fp32 restatement of sq_box_iou), the same for iou_sum per tp, the "
        "lanes left out as fragile and the events counted; integer outputs, counts and last_id are compared exactly")


def _record(case, **figures):
    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data["cases"][case] = figures
    merge_parity("score_parity.json", lambda: {"note": NOTE, "cases": {}}, update)


_handles = {}


def _handle(c):
    key = (c.wide, c.N)
    if key not in _handles:
        _handles[key] = open_handle(_capi.WIDE_LIB_PATH if c.wide else None, SC.HW, k_particles=2, n_steps_per_image=c.N, n_what=6)
    return _handles[key]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """The case's inputs on the host and on the device, the reference and the lanes compared: made once, never written to."""
    c = SC.CASES[i]
    x = SC.make(c)
    d = {k: torch.from_numpy(np.array(v)).cuda() for k, v in x.items()}
    ref = R.score(iou_min=c.iou_min, **x)
    first = R.fragile_from(ref.iou, x["presence"], x["map_count"], x["truth_present"], x["truth_valid"], c.iou_min)
    tol = 4.0 * R.iou32_error(x["truth_box"], x["box"])
    return x, d, ref, first, tol


def _state(G):
    return dict(counts=torch.zeros((SC.B, 9), dtype=torch.int64, device="cuda"), iou_sum=torch.zeros(SC.B, dtype=torch.float64, device="cuda"),
                last_id=torch.full((SC.B, G), -1, dtype=torch.int32, device="cuda"))


def _run(c, d, state, frames=slice(None), fields=_capi.SCORE_FIELDS):
    """One launch over ``frames`` of the case, continuing ``state`` in place; returns the per-frame outputs asked for."""
    lib, h = _handle(c)
    x = {k: v[frames].contiguous() for k, v in d.items()}
    T = x["map_count"].shape[0]
    shapes = _capi.score_shapes(T, SC.B, c.G)
    o = {n: torch.full(shapes[n], -7, dtype=torch.int32 if n in _capi.SCORE_INT_FIELDS else torch.float32, device="cuda") for n in fields}
    sc = _capi.SqairLaneScore(iou_min=c.iou_min, G=c.G, truth_box=x["truth_box"].data_ptr(), truth_present=x["truth_present"].data_ptr(),
                              truth_valid=x["truth_valid"].data_ptr(), **{n: t.data_ptr() for n, t in state.items()},
                              **{n: t.data_ptr() for n, t in o.items()})
    s = torch.cuda.current_stream()
    rc = lib.sqair_lane_score_test(h, x["box"].data_ptr(), x["presence"].data_ptr(), x["obj_id"].data_ptr(), x["map_count"].data_ptr(),
                                   T, SC.B, C.byref(sc), C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}


@pytest.mark.parametrize("i", range(len(SC.CASES)), ids=[SC.case_id(c) for c in SC.CASES])
def test_score_kernel_against_fp64(i):
    c = SC.CASES[i]
    x, d, ref, first, tol = _inputs(i)
    state = _state(c.G)
    got = _run(c, d, state)
    counts, iou_sum, last_id = (state[n].cpu().numpy() for n in ("counts", "iou_sum", "last_id"))
    whole = first == SC.T                                          # lanes compared to the end
    upto = np.arange(SC.T)[:, None] < first[None, :]               # [T, B]: frames before a lane's first fragile one
    left_out = int((~whole).sum())
    print(SC.case_id(c), "lanes left out as fragile:", left_out, "of", SC.B)
    assert left_out <= SC.FRAGILE_CAP * SC.B
    for n in INT_OUT:
        assert np.array_equal(got[n][upto], getattr(ref, n)[upto]), (n, np.argwhere(got[n][upto] != getattr(ref, n)[upto])[:4])
    assert np.array_equal(counts[whole], ref.counts[whole]), np.argwhere(counts != ref.counts)[:4]
    assert np.array_equal(last_id[whole], ref.last_id[whole])
    err = float(np.abs(got["match_iou"].astype(np.float64) - ref.match_iou)[upto].max())
    err_sum = float((np.abs(iou_sum - ref.iou_sum) / np.maximum(ref.counts[:, 3], 1))[whole].max())
    tot = dict(zip(R.COUNTS, counts.sum(0).tolist()))
    print(SC.case_id(c), "match_iou: largest error {:.3g}, iou_sum per tp {:.3g}; allowed {:.3g}".format(err, err_sum, tol), tot)
    _record(SC.case_id(c), match_iou=err, iou_sum_per_tp=err_sum, allowed=tol, lanes=SC.B, left_out=left_out, **tot)
    assert tol < 1e-5 and err <= tol and err_sum <= tol
    assert (np.abs(iou_sum - ref.iou_sum) <= tol * ref.counts[:, 3])[whole].all()
    # unscored frames: -1 / 0; the non-finite lane and the lane without truth
    unscored = (x["truth_valid"] == 0) | (x["map_count"] == -1)
    assert all((got[n][unscored] == -1).all() for n in INT_OUT) and not got["match_iou"][unscored].any()
    assert counts[SC.NAN_LANE, 1] == SC.T - SC.NAN_FROM and not counts[SC.INVALID_LANE].any() and (last_id[SC.INVALID_LANE] == -1).all()
    assert min(tot.values()) > 0


@pytest.mark.parametrize("i", [0, 5], ids=[SC.case_id(SC.CASES[i]) for i in (0, 5)])
def test_two_passes_equal_one_and_the_outputs_are_optional(i):
    c = SC.CASES[i]
    _, d, _, _, _ = _inputs(i)
    one = _state(c.G)
    full = _run(c, d, one)
    two = _state(c.G)
    a, b = _run(c, d, two, slice(0, 3)), _run(c, d, two, slice(3, 6))
    for n in _capi.SCORE_FIELDS:
        assert np.array_equal(np.concatenate([a[n], b[n]]).view(np.int32), full[n].view(np.int32)), n
    for n in one:
        assert torch.equal(one[n], two[n]), n
    for fields in ((), ("match_iou",), ("truth_match", "fp")):
        st = _state(c.G)
        part = _run(c, d, st, fields=fields)
        assert all(np.array_equal(part[n].view(np.int32), full[n].view(np.int32)) for n in fields)
        assert all(torch.equal(one[n], st[n]) for n in one), fields
