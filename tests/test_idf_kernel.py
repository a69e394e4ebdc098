"""-m gpu: the IDF1 accumulation kernel (k_lane_idf, through sqair_lane_idf_test) against the reference of tests/idf_ref.py, on caller
buffers, for the cases of tests/idf_cases.py: 200 lanes, T = 8, (G, N, P) = (4, 4, 8) -- overflowing --, (4, 4, 32), (1, 4, 1),
(3, 4, 5) and (16, 14, 64) on the wide library -- every thread of the workgroup that owns a pair has one there --, iou_min 0.5 and 0.3.

Everything the kernel writes is an integer: the whole table and ``totals`` are compared exactly on the lanes that are not fragile --
a lane is fragile when a present pair's float64 IoU lies within four times the measured error of an fp32 restatement of sq_box_iou
of iou_min (tests/idf_ref.py: fragile_from), at most 1 % of the lanes; tests/test_idf_ref.py holds the same inputs to that cap from
the reference alone.  Also here: two passes of four frames give the bits of one pass of eight, a captured graph replayed equals
eager calls, and the solve of the accumulated table gives the reference's twelve figures.  With SQAIR_PARITY_DIR set the cases are
recorded in idf_parity.json there (the copy under profiles/ is such a file)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import idf_cases as IC
from tests import idf_ref as R
from tests import score_ref as SR
from tests.abi_host import open_handle
from tests.idf_cases import record, run_solve, struct, to_device

pytestmark = pytest.mark.gpu

INPUTS = ("box", "presence", "ids", "map_count", "truth_box", "truth_present", "truth_valid", "truth_match")
HW = IC.SC.HW
_handles = {}


def _handle(c):
    key = (c.wide, c.N)
    if key not in _handles:
        _handles[key] = open_handle(_capi.WIDE_LIB_PATH if c.wide else None, HW, k_particles=2, n_steps_per_image=c.N, n_what=6)
    return _handles[key]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """The case's inputs on the host and on the device, the reference table and the lanes compared: made once, never written to."""
    c = IC.CASES[i]
    x = IC.make(c)
    d = {k: torch.from_numpy(np.array(x[k])).cuda() for k in INPUTS}
    ref = R.accumulate(R.new_table(IC.B, c.G, c.P), *[x[k] for k in INPUTS], c.iou_min)
    near = 4.0 * SR.iou32_error(x["truth_box"], x["box"])
    first = R.fragile_from(SR.iou_table(x["truth_box"], x["box"]), x["presence"], x["map_count"], x["truth_present"], x["truth_valid"],
                           c.iou_min, near)
    return x, d, ref, first == IC.T


def _launch(c, d, table, frames=slice(None), stream=None, x=None):
    """One launch over ``frames`` of the case on ``stream`` (default: the current one), continuing the device table ``table`` in
    place; ``x``: the frames' contiguous inputs when they were cut before (a capture allocates nothing).  Returns them: the caller
    keeps them alive until the stream has run."""
    lib, h = _handle(c)
    x = x or {k: v[frames].contiguous() for k, v in d.items()}
    T = x["map_count"].shape[0]
    sc = _capi.SqairLaneScore(iou_min=c.iou_min, G=c.G, truth_box=x["truth_box"].data_ptr(), truth_present=x["truth_present"].data_ptr(),
                              truth_valid=x["truth_valid"].data_ptr(), truth_match=x["truth_match"].data_ptr())
    rc = lib.sqair_lane_idf_test(h, x["box"].data_ptr(), x["presence"].data_ptr(), x["ids"].data_ptr(), x["map_count"].data_ptr(), T, IC.B,
                                 C.byref(sc), C.byref(struct(table, c.P)), C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    return x


def _fresh(c):
    return to_device(R.new_table(IC.B, c.G, c.P))


@pytest.mark.parametrize("i", range(len(IC.CASES)), ids=[IC.case_id(c) for c in IC.CASES])
def test_idf_kernel_against_the_reference_and_the_solve_of_its_table(i):
    c = IC.CASES[i]
    x, d, ref, whole = _inputs(i)
    table = _fresh(c)
    keep = _launch(c, d, table)
    torch.cuda.synchronize()
    del keep
    got = {n: v.cpu().numpy() for n, v in table.items()}
    left_out = int((~whole).sum())
    print(IC.case_id(c), "lanes left out as fragile:", left_out, "of", IC.B)
    assert left_out <= IC.FRAGILE_CAP * IC.B
    for n in ref:
        a, b = got[n][whole], ref[n][whole]
        if n in ("overlap", "col_frames"):      # (the words of a free column are never read)
            used = ref["col_id"][whole] >= 0
            a, b = (np.where(used[:, None, :], a, 0), np.where(used[:, None, :], b, 0)) if n == "overlap" else (np.where(used, a, 0), np.where(used, b, 0))
        assert np.array_equal(a, b), (n, np.argwhere(a != b)[:4])
    # untouched: the lane without a valid frame; counted: frames, overflow
    assert (got["col_id"][IC.SC.INVALID_LANE] == -1).all() and got["frames"][IC.SC.INVALID_LANE] == 0
    assert got["frames"][IC.SC.NAN_LANE] == int(x["truth_valid"][:IC.SC.NAN_FROM, IC.SC.NAN_LANE].sum())
    # then the solve: the twelve figures of every compared lane
    open_, assign = run_solve("wide" if c.wide else "product", table, c.G, c.P)
    _, ref_open = R.solve(ref)
    assert np.array_equal(open_[whole], ref_open[whole]), np.argwhere(open_ != ref_open)[:4]
    idtp = R.TOTALS.index("idtp")
    for b in np.flatnonzero(whole):
        R.check_assign(ref, b, assign[b], int(ref_open[b, idtp]))
    tot = dict(zip(R.TOTALS, (open_[whole] + got["totals"][whole]).sum(0).tolist()))
    print(IC.case_id(c), tot, R.pooled(open_[whole] + got["totals"][whole]))
    record("accumulate", IC.case_id(c), lanes=IC.B, left_out=left_out, **tot)
    assert tot["idtp"] > 0 and tot["idfn"] > 0 and tot["idfp"] > 0 and tot["overflow_ids"] > 0


@pytest.mark.parametrize("i", [0, 6, 8], ids=[IC.case_id(IC.CASES[i]) for i in (0, 6, 8)])
def test_two_passes_of_four_frames_equal_one_of_eight_and_graph_equals_eager(i):
    c = IC.CASES[i]
    _, d, _, _ = _inputs(i)
    one = _fresh(c)
    _launch(c, d, one)
    two = _fresh(c)
    a, b = _launch(c, d, two, slice(0, 4)), _launch(c, d, two, slice(4, 8))
    torch.cuda.synchronize()
    for n in one:
        assert torch.equal(one[n], two[n]), n
    # a captured graph of the one launch (sqair_capture_begin / _end) over the second half, replayed on the table the first half left
    lib, h = _handle(c)
    three = _fresh(c)
    first = _launch(c, d, three, slice(0, 4))
    second = {k: v[4:8].contiguous() for k, v in d.items()}
    torch.cuda.synchronize()
    snapshot = {n: v.clone() for n, v in three.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    _launch(c, d, three, stream=side, x=second)
    assert lib.sqair_capture_end(h, ss, 3) == 1, lib.sqair_last_error(h)      # one launch per call: one kernel node
    torch.cuda.synchronize()
    for n, v in snapshot.items():                # (the capture launched nothing)
        assert torch.equal(three[n], v), n
    assert lib.sqair_capture_launch(h, 3, ss) == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    del a, b, first
    for n in one:
        assert torch.equal(one[n], three[n]), n
