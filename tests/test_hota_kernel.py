"""-m gpu: the HOTA append kernel (k_lane_hota, through sqair_lane_hota_test) against the reference of tests/hota_ref.py, on caller
buffers, for the cases of tests/hota_cases.py: 24 lanes, T = 40, (G, N, P, L) = (4, 4, 32, 64), (1, 4, 8, 16) and (16, 14, 64, 32) on
the wide library.

``log_col``, ``log_row``, ``col_id``, ``frames``, ``dropped_frames`` and ``totals_c`` are compared exactly.  ``log_q`` holds -1 in
exactly the reference's cells and lies within +-1 of the float64 q elsewhere: the device's IoU is fp32, whose error the score's
parity profile puts near 3e-8, well under one unit of 2^-20, so only a rounding boundary can move q, and by one.  The records not in
use are never written.  Also here: the same frames in split passes give the bits of one pass, a captured graph replayed twice equals
two eager calls, and the solve of the kernel's OWN log gives the reference's figures on that log."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import hota_cases as HC
from tests import hota_ref as R
from tests.hota_cases import close_enough, handle, judged, run_solve, struct, to_device

pytestmark = pytest.mark.gpu

EXACT = ("col_id", "log_col", "log_row", "frames", "dropped_frames", "totals_c")
SPLITS = (7, 8, 1, 24)          # T = 40 in four passes, the log filling up inside one of them


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """The case's inputs on the host and on the device and the reference's log: made once, never written to."""
    c = HC.CASES[i]
    x = HC.make(c)
    d = {k: torch.from_numpy(np.array(x[k])).cuda() for k in HC.INPUTS}
    ref = R.append(R.new_log(HC.B, c.G, c.N, c.P, c.L), *[x[k] for k in HC.INPUTS])
    return x, d, ref


def _lib(c):
    return "wide" if c.wide else "product"


def _fresh(c):
    return to_device(R.new_log(HC.B, c.G, c.N, c.P, c.L), c.G, c.P)


def _launch(c, d, log, frames=slice(None), stream=None, x=None):
    """One launch over ``frames`` of the case on ``stream`` (default: the current one), continuing the device log in place; ``x``:
    the frames' contiguous inputs when they were cut before (a capture allocates nothing).  Returns them: the caller keeps them
    alive until the stream has run."""
    lib, h = handle(_lib(c), c.N)
    x = x or {k: v[frames].contiguous() for k, v in d.items()}
    sc = _capi.SqairLaneScore(iou_min=0.5, G=c.G, truth_box=x["truth_box"].data_ptr(), truth_present=x["truth_present"].data_ptr(),
                              truth_valid=x["truth_valid"].data_ptr())
    rc = lib.sqair_lane_hota_test(h, x["box"].data_ptr(), x["presence"].data_ptr(), x["ids"].data_ptr(), x["map_count"].data_ptr(),
                                  x["map_count"].shape[0], HC.B, C.byref(sc), C.byref(struct(log, c.P, c.L)),
                                  C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    return x


@pytest.mark.parametrize("i", range(len(HC.CASES)), ids=[HC.case_id(c) for c in HC.CASES])
def test_append_against_the_reference_and_the_solve_of_its_own_log(i):
    c = HC.CASES[i]
    x, d, ref = _inputs(i)
    log = _fresh(c)
    keep = _launch(c, d, log)
    torch.cuda.synchronize()
    del keep
    got = {n: v.cpu().numpy() for n, v in log.items()}
    for n in EXACT:
        assert np.array_equal(got[n], ref[n]), (n, np.argwhere(got[n] != ref[n])[:4])
    none = ref["log_q"] < 0                                    # -1 in a record in use, -7 in one that is not: the same cells, the same words
    assert np.array_equal(got["log_q"][none], ref["log_q"][none])
    off = np.abs(got["log_q"].astype(np.int64) - ref["log_q"])[~none]
    print(HC.case_id(c), "pairs", off.size, "q off by one", int((off == 1).sum()), "worst", int(off.max()))
    assert off.max() <= 1
    assert (got["totals_i"] == 0).all() and (got["totals_f"] == 0).all() and (got["work"] == 12345).all()      # the append's are totals_c alone
    # what the cases are for
    frames, dropped = got["frames"], got["dropped_frames"]
    assert frames[HC.INVALID_LANE] == 0 and (got["col_id"][HC.INVALID_LANE] == -1).all()
    assert frames[HC.NAN_LANE] == HC.NAN_FROM and dropped[HC.NAN_LANE] == 0
    assert got["totals_c"][:, 3].sum() > 0 and (got["log_col"] == -2).any()
    assert (dropped > 0).any() == (c.L < HC.T) and (frames <= c.L).all()
    # then the solve of this very log
    mine = {n: got[n] for n in ref}
    solved = run_solve(_lib(c), log, c.G, c.N, c.P, c.L)
    _, oi, of, oc, n, _ = judged(mine, solved)
    assert np.array_equal(solved["open_i"], oi) and np.array_equal(solved["open_c"], oc) and close_enough(solved["open_f"], of)
    assert n == int(frames.sum()) and oi[:, :, 0].sum() > 0


@pytest.mark.parametrize("i", range(len(HC.CASES)), ids=[HC.case_id(c) for c in HC.CASES])
def test_split_passes_equal_one_pass_and_a_graph_replayed_twice_equals_two_eager_calls(i):
    c = HC.CASES[i]
    _, d, _ = _inputs(i)
    one = _fresh(c)
    keep = [_launch(c, d, one)]
    two, at = _fresh(c), 0
    for n in SPLITS:
        keep.append(_launch(c, d, two, slice(at, at + n)))
        at += n
    assert at == HC.T
    torch.cuda.synchronize()
    for n in one:
        assert torch.equal(one[n], two[n]), n
    # the same eight frames twice: eagerly, and as one captured launch (sqair_capture_begin / _end) replayed twice
    lib, h = handle(_lib(c), c.N)
    eager, graph = _fresh(c), _fresh(c)
    part = {k: v[4:12].contiguous() for k, v in d.items()}
    keep += [_launch(c, d, eager, x=part), _launch(c, d, eager, x=part)]
    torch.cuda.synchronize()
    snapshot = {n: v.clone() for n, v in graph.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    _launch(c, d, graph, stream=side, x=part)
    assert lib.sqair_capture_end(h, ss, 3) == 1, lib.sqair_last_error(h)      # one launch per call: one kernel node
    torch.cuda.synchronize()
    for n, v in snapshot.items():                # (the capture launched nothing)
        assert torch.equal(graph[n], v), n
    for _ in range(2):
        assert lib.sqair_capture_launch(h, 3, ss) == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    del keep
    for n in eager:
        assert torch.equal(eager[n], graph[n]), n
    assert (eager["frames"] > 8).any()
