"""-m gpu: the track log's two kernels on caller buffers, against the reference of tests/tracklog_ref.py on the cases of
tests/tracklog_cases.py (at most 8 lanes of 12 frames; what each case exercises is listed there).

The append (k_lane_tracklog, through sqair_lane_tracklog_test): the log's bytes equal the reference's in every case, two passes
leave the bytes of one, a captured graph replayed twice leaves the bytes of eager calls.  The solve (k_lane_tracklog_smooth, through
sqair_lane_tracklog_smooth): ``track_id``, ``n_tracks``, ``len0``, ``frame_index``, ``state`` and ``size`` are exact; ``filt`` and
``smooth`` lie within a bar that is MEASURED -- per case four times the largest error of the fp32 restatement of the header against
float64 (tests/tracklog_ref.py), never anything the kernel gave --; a replayed solve gives the eager solve's bits; it writes nothing
but its outputs and its scratch.  And the bit check that holds the solve's filter and the identity's together: with
sqair_lane_identity_motion_test run on the same scene and scalars, the solve's filtered velocity has the bits of the motion kernel's
``velocity`` at every seen frame after the first of every column born inside the window.  With SQAIR_PARITY_DIR set the bars and the
kernel's own error go into tracklog_parity.json there (the copy under profiles/ is such a file)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tracklog_cases as TC
from tests import tracklog_ref as R

pytestmark = pytest.mark.gpu

NAMES = list(TC.CASES)
EXACT = ("track_id", "n_tracks", "len0", "frame_index", "state", "size")


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _log_equal(d, log):
    return [n for n in R.FIELDS if not np.array_equal(_bytes(d[n].cpu().numpy()), _bytes(log[n]))]


def _append(name, split=None):
    """The append kernel over the case's frames in its passes (or ``split``); returns the device log."""
    c = TC.CASES[name]
    x = TC.make(name)
    lib, h = TC.handle(c.N, c.wide)
    d = TC.to_device(R.new_log(x["best_row"].shape[1], c.L, c.N))
    dx = TC.to_device(x)
    for lo, hi in (split or TC.passes(name)):
        TC.run_append(lib, h, {k: v[lo:hi].contiguous() for k, v in dx.items()}, d, c.L)
    torch.cuda.synchronize()
    return d


@pytest.mark.parametrize("name", NAMES)
def test_the_appends_bytes_equal_the_references(name):
    _, log, _ = TC.reference(name)
    d = _append(name)
    assert not _log_equal(d, log), _log_equal(d, log)
    assert d["count"].dtype == torch.int64 and d["count"].tolist() == log["count"].tolist()


@pytest.mark.parametrize("name", ["a", "f", "g"])
def test_two_passes_equal_one(name):
    n = sum(TC.CASES[name].passes)
    one, two, singles = _append(name, [(0, n)]), _append(name, [(0, 5), (5, n)]), _append(name, [(t, t + 1) for t in range(n)])
    for k in R.FIELDS:
        assert torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k
        assert torch.equal(one[k].view(torch.uint8), singles[k].view(torch.uint8)), k
    assert not _log_equal(one, TC.reference(name)[1])


def test_a_replayed_graph_leaves_the_bytes_of_eager_calls():
    """One launch of six frames captured once and replayed twice, on the first and then on the second half of case a, against two
    eager launches: count is read and advanced on the device, so a replay continues the ring as an eager call does."""
    c = TC.CASES["a"]
    lib, h = TC.handle(c.N)
    want = _append("a", [(0, 6), (6, 12)])
    dx = TC.to_device(TC.make("a"))
    halves = [{k: v[f].contiguous() for k, v in dx.items()} for f in (slice(0, 6), slice(6, 12))]
    x = {k: v.clone() for k, v in halves[0].items()}           # the graph's input buffers
    d = TC.to_device(R.new_log(dx["best_row"].shape[1], c.L, c.N))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    TC.run_append(lib, h, x, d, c.L, stream=side)
    assert lib.sqair_capture_end(h, ss, 2) == 1, lib.sqair_last_error(h)      # one launch: one kernel node
    torch.cuda.synchronize()
    assert not d["count"].any() and not d["log_valid"].any()                  # (a capture launches nothing)
    for half in halves:
        for k in x:
            x[k].copy_(half[k])
        torch.cuda.synchronize()
        assert lib.sqair_capture_launch(h, 2, ss) == 0, lib.sqair_last_error(h)
        torch.cuda.synchronize()
    for k in R.FIELDS:
        assert torch.equal(d[k].view(torch.uint8), want[k].view(torch.uint8)), k


def _solve(name, d=None, stream=None, buffers=None):
    c = TC.CASES[name]
    _, log, _ = TC.reference(name)
    lib, h = TC.handle(c.N, c.wide)
    d = TC.to_device(log) if d is None else d
    out, work = buffers or TC.solve_buffers(lib, c.lag, d["count"].shape[0], c.C, c.N)
    TC.run_smooth(lib, h, d, c.L, c.lag, c.C, c.N, out, work, stream=stream)
    torch.cuda.synchronize()
    return d, out, work


@pytest.mark.parametrize("name", NAMES)
def test_the_solve_against_the_reference(name):
    c = TC.CASES[name]
    _, log, ref = TC.reference(name)
    d, out, _ = _solve(name)
    assert not _log_equal(d, log)                                            # the log is read, not written
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in EXACT:
        want = getattr(ref, k)
        assert got[k].dtype == want.dtype and np.array_equal(_bytes(got[k]), _bytes(want)), (k, np.argwhere(got[k] != want)[:6])
    bars = R.bars(ref.err)
    errs = dict(filt=float(np.abs(got["filt"] - ref.filt).max()), smooth=float(np.abs(got["smooth"] - ref.smooth).max()))
    same32 = dict(filt=bool(np.array_equal(_bytes(got["filt"]), _bytes(ref.filt32))),
                  smooth=bool(np.array_equal(_bytes(got["smooth"]), _bytes(ref.smooth32))))
    print(name, "bars", bars, "the kernel's error against float64", errs, "the restatement's bits", same32)
    TC.record("cases", name, shape=dict(N=c.N, C=c.C, L=c.L, lag=c.lag, lanes=int(ref.n_tracks.shape[0])), bars=bars, kernel_error=errs,
              restatement_bits=same32, tracks=int(ref.n_tracks.sum()), states=[int((ref.state == k).sum()) for k in range(4)])
    assert got["filt"].dtype == got["smooth"].dtype == np.float32 and np.isfinite(got["filt"]).all() and np.isfinite(got["smooth"]).all()
    for k in errs:
        assert errs[k] <= bars[k], (k, errs[k], bars[k])
    stepped = (ref.state == R.SEEN) | (ref.state == R.GAP)
    assert not got["filt"][~stepped].any() and not got["smooth"][~stepped].any()          # 0 where the state is 0 or 3


def test_a_replayed_solve_gives_the_eager_solves_bits():
    c = TC.CASES["a"]
    lib, h = TC.handle(c.N)
    _, eager, _ = _solve("a")
    d = TC.to_device(TC.reference("a")[1])
    buffers = TC.solve_buffers(lib, c.lag, d["count"].shape[0], c.C, c.N)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    TC.run_smooth(lib, h, d, c.L, c.lag, c.C, c.N, *buffers, stream=side)
    assert lib.sqair_capture_end(h, ss, 1) == 1, lib.sqair_last_error(h)      # one launch: one kernel node
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in buffers[0].values())                  # (a capture launches nothing)
    for _ in range(2):
        for t in buffers[0].values():
            t.fill_(-7)
        torch.cuda.synchronize()
        assert lib.sqair_capture_launch(h, 1, ss) == 0, lib.sqair_last_error(h)
        torch.cuda.synchronize()
        for k, t in buffers[0].items():
            assert torch.equal(t.view(torch.uint8), eager[k].view(torch.uint8)), k


@pytest.mark.parametrize("name", ["d", "f", "g", "h"])
def test_the_forward_velocity_has_the_bits_of_the_motion_kernels(name):
    """The motion kernel's own lane_id and track_len go through the append kernel, the solve runs on that log with the same scalars:
    no reference in between, bits against bits."""
    c = TC.CASES[name]
    assert c.L >= c.lag >= sum(c.passes)                                    # the window holds every frame
    mk = TC.motion_kernel(name)
    x = TC.make(name)
    lib, h = TC.handle(c.N, c.wide)
    B = x["best_row"].shape[1]
    d = TC.to_device(R.new_log(B, c.L, c.N))
    TC.run_append(lib, h, TC.to_device(dict(lane_id=mk["lane_id"], track_len=mk["track_len"], best_row=x["best_row"], box=x["box"])), d, c.L)
    out, work = TC.solve_buffers(lib, c.lag, B, c.C, c.N)
    TC.run_smooth(lib, h, d, c.L, c.lag, c.C, c.N, out, work)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    n = 0
    for b in range(B):
        for col in np.flatnonzero(got["len0"][b] == 1):
            for f in np.flatnonzero(got["state"][:, b, col] == R.SEEN)[1:]:
                t = int(got["frame_index"][f, b])
                j = int(np.flatnonzero(mk["lane_id"][t, b] == got["track_id"][b, col])[0])
                a, w = got["filt"][f, b, col, :, 1], mk["velocity"][t, b, j]
                assert np.array_equal(a.view(np.uint32), w.view(np.uint32)), (b, col, f, a, w)
                n += 1
    print(name, "velocities compared as bits", n)
    assert n > 0
