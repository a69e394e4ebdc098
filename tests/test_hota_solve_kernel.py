"""-m gpu: the HOTA solve alone (k_lane_hota_solve, through sqair_lane_hota_solve) on given integer logs -- the logs the reference's
append (tests/hota_ref.py) makes of the cases of tests/hota_cases.py -- on both libraries; tests/test_hota_kernel.py runs it on the
append kernel's own logs through the same helpers.

Optimal assignments tie and the header states no rule among them, so every record's ``match`` is JUDGED -- one-to-one, only pairs
of weight >= 0, its integer total SciPy's optimum of the reference's table exactly: the weights are integers, there is no slack --
and then IMPOSED on the reference.  With it ``open_i`` and ``open_c`` (and the totals after a close) are exact; the doubles agree
within 1e-12 relative: at most G P = 1024 terms of relative rounding 2^-53 each, of which 1e-12 is about eight times the sum.
Without ``close`` nothing but ``work`` changes; ``close`` frees those lanes and only those and accumulates; the outputs are
optional.  With SQAIR_PARITY_DIR set the share of records whose device matching is not SciPy's own, and the HOTA difference that
makes, go into hota_parity.json there (recorded, not gated)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import hota_cases as HC
from tests import hota_ref as R
from tests.abi_host import LANE_LIBS as LIBS
from tests.hota_cases import close_enough, handle, judged, record, run_solve, struct, to_device

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def reference_log(i):
    """The reference's log of case i after all its frames; made once, never written to."""
    c = HC.CASES[i]
    x = HC.make(c)
    log = R.append(R.new_log(HC.B, c.G, c.N, c.P, c.L), *[x[k] for k in HC.INPUTS])
    rng = np.random.default_rng(c.seed + 2)
    log["totals_i"][:] = rng.integers(0, 1 << 40, log["totals_i"].shape)        # a close adds to what is there
    log["totals_f"][:] = rng.uniform(0, 1e6, log["totals_f"].shape)
    log["totals_c"][:, :3] = rng.integers(0, 1 << 40, (HC.B, 3))
    for a in log.values():
        a.setflags(write=False)
    return log


def changed(d, log):
    return [n for n in log if not np.array_equal(d[n].cpu().numpy(), log[n], equal_nan=True)]


@pytest.mark.parametrize("lib_name", list(LIBS))
@pytest.mark.parametrize("i", range(len(HC.CASES)), ids=[HC.case_id(c) for c in HC.CASES])
def test_solve_against_the_reference_on_its_own_matching(i, lib_name):
    c = HC.CASES[i]
    log = reference_log(i)
    d = to_device(log, c.G, c.P)
    got = run_solve(lib_name, d, c.G, c.N, c.P, c.L)
    assert not changed(d, log)                                              # without close nothing changes
    _, oi, of, oc, n, differ = judged(log, got)
    assert np.array_equal(got["open_i"], oi), np.argwhere(got["open_i"] != oi)[:6]
    assert np.array_equal(got["open_c"], oc), np.argwhere(got["open_c"] != oc)[:6]
    assert close_enough(got["open_f"], of), np.abs(got["open_f"] - of).max()
    # recorded, not gated: how often the device's optimal matching is not SciPy's, and what that does to HOTA
    _, si, sf, _, _, _ = R.solve(log)
    dev, sci = R.figures(oi.sum(0), of.sum(0)), R.figures(si.sum(0), sf.sum(0))
    print(HC.case_id(c), lib_name, "records", n, "matched otherwise than SciPy", differ, "HOTA", dev["hota"], "SciPy's", sci["hota"])
    record("device_vs_scipy", "{}_{}".format(HC.case_id(c), lib_name), records=n, records_matched_otherwise=differ,
           share=differ / float(n), hota=dev["hota"], hota_scipy=sci["hota"], hota_difference=abs(dev["hota"] - sci["hota"]))
    assert n > 0 and oi[:, :, 0].sum() > 0 and oi[:, :, 1].sum() > 0 and oi[:, :, 2].sum() > 0
    assert oc[:, 2].sum() > 0 or c.L >= HC.T                                # dropped frames where the clip is longer than the log


@pytest.mark.parametrize("lib_name", list(LIBS))
@pytest.mark.parametrize("i", [0, 2], ids=[HC.case_id(HC.CASES[i]) for i in (0, 2)])
def test_close_frees_those_lanes_only_and_the_totals_add_up(i, lib_name):
    c = HC.CASES[i]
    log = reference_log(i)
    d = to_device(log, c.G, c.P)
    close = (np.arange(HC.B) % 3 == 1).astype(np.int32)
    got = run_solve(lib_name, d, c.G, c.N, c.P, c.L, close=close)
    after, oi, of, oc, _, _ = judged(log, got, close=close)
    now = {n: v.cpu().numpy() for n, v in d.items()}
    for n in ("col_id", "log_q", "log_col", "log_row", "frames", "dropped_frames", "totals_i", "totals_c"):
        assert np.array_equal(now[n], after[n]), n
    assert close_enough(now["totals_f"], after["totals_f"])
    assert np.array_equal(got["open_i"], oi) and np.array_equal(got["open_c"], oc) and close_enough(got["open_f"], of)
    kept = close == 0
    assert all(np.array_equal(now[n][kept], log[n][kept]) for n in log)
    assert (now["col_id"][~kept] == -1).all() and not now["frames"][~kept].any() and not now["dropped_frames"][~kept].any()
    assert np.array_equal(now["totals_i"][~kept], log["totals_i"][~kept] + oi[~kept])
    assert np.array_equal(now["totals_c"][~kept], log["totals_c"][~kept] + oc[~kept])
    # a second close of every lane, no outputs: the freed lanes add an empty clip -- nothing --, the others their figures
    assert run_solve(lib_name, d, c.G, c.N, c.P, c.L, close=np.ones(HC.B, np.int32), want=()) == {}
    now = {n: v.cpu().numpy() for n, v in d.items()}
    assert np.array_equal(now["totals_i"], log["totals_i"] + oi) and np.array_equal(now["totals_c"], log["totals_c"] + oc)
    assert close_enough(now["totals_f"], log["totals_f"] + of) and (now["col_id"] == -1).all() and not now["frames"].any()
    # each output alone
    for k in ("open_i", "open_f", "open_c", "match"):
        e = to_device(log, c.G, c.P)
        one = run_solve(lib_name, e, c.G, c.N, c.P, c.L, want=(k,))
        assert not changed(e, log) and list(one) == [k] and np.array_equal(one[k], got[k]), k      # (the doubles too: a fixed order)


def test_a_solve_in_a_captured_graph_equals_the_eager_one():
    c = HC.CASES[0]
    log = reference_log(0)
    eager = run_solve("product", to_device(log, c.G, c.P), c.G, c.N, c.P, c.L)
    lib, h = handle("product")
    d = to_device(log, c.G, c.P)
    shapes = _capi.hota_solve_shapes(HC.B, c.G, c.L)
    out = {k: torch.full(shapes[k], -7, dtype=getattr(torch, _capi.field_dtype("sqair_lane_hota_solve", k)), device="cuda")
           for k in ("open_i", "open_f", "open_c", "match")}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    assert lib.sqair_lane_hota_solve(h, C.byref(struct(d, c.P, c.L)), c.G, c.N, HC.B, None, out["open_i"].data_ptr(), out["open_f"].data_ptr(),
                                     out["open_c"].data_ptr(), out["match"].data_ptr(), ss) == 0, lib.sqair_last_error(h)
    assert lib.sqair_capture_end(h, ss, 3) == 1, lib.sqair_last_error(h)      # one launch: one kernel node
    torch.cuda.synchronize()
    assert (out["open_c"] == -7).all()                                        # (the capture launched nothing)
    for _ in range(2):
        assert lib.sqair_capture_launch(h, 3, ss) == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    for k, v in out.items():
        assert np.array_equal(v.cpu().numpy(), eager[k]), k                   # the doubles too: one thread, a fixed order
