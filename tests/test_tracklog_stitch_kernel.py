"""-m gpu: k_lane_tracklog_stitch through sqair_lane_tracklog_stitch on caller tensors, fed the kernel's OWN solve outputs
(k_lane_tracklog_smooth on the case's log: its table and its ``work``), against the float64 reference of tests/tracklog_stitch_ref.py
-- the cases of tests/tracklog_stitch_cases.py; what each exercises is listed there.

Every integer output is exactly the reference's: link_next, link_gap, root, n_links, the stitched track_id, n_tracks, len0, state,
frame_index and work_out.  link_d2 is held to float64 within four times the MEASURED error of the fp32 restatement of the header
(the reference's, per case, never anything the kernel gave), the stitched filt and smooth within the solve's own bars
(tests/tracklog_ref.py: ``bars``, of the stitched table).  For the relabelled cases the stitched table is, bit for bit and device
against device, what k_lane_tracklog_smooth writes for the log never relabelled: that needs no tolerance.  Every output is prefilled
with -7, so every word must be written; the call writes nothing but its outputs; a captured graph replayed twice gives the eager call's
bits; sqair_lane_tracklog_score on the stitched table gives the counters the reference gave.  With SQAIR_PARITY_DIR set the bars and
the kernel's own errors go into tracklog_stitch_parity.json there (the copy under profiles/ is such a file)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tracklog_cases as TC
from tests import tracklog_ref as R
from tests import tracklog_score_cases as SCC
from tests import tracklog_score_ref as SCR
from tests import tracklog_stitch_cases as SC

pytestmark = pytest.mark.gpu

INTS = ("track_id", "n_tracks", "len0", "frame_index", "state")
LINK_INTS = ("link_next", "link_gap", "root", "n_links")
BIT_FIELDS = ("state", "size", "filt", "smooth", "track_id", "len0", "n_tracks")
K = {n: i for i, n in enumerate(SCR.COUNTS)}
FILLED = SCR.VIEWS.index("smooth_filled")
_solved = {}


def _solve(name, plain=False):
    """(lib, h, the device log, the kernel's solve of it on the device: table and work), once per log."""
    c = SC.make(name)
    if (name, plain) not in _solved:
        lib, h = TC.handle(2)   # (the handle gives the error text only: N is the calls' argument, 16 in limit)
        d = TC.to_device(c.plain if plain else c.log)
        out, work = TC.solve_buffers(lib, c.lag, d["count"].shape[0], c.C, c.N)
        TC.run_smooth(lib, h, d, c.L, c.lag, c.C, c.N, out, work)
        torch.cuda.synchronize()
        _solved[name, plain] = lib, h, d, out, work
    return _solved[name, plain]


def _stitch(name, stream=None, buffers=None):
    c = SC.make(name)
    lib, h, d, table, work = _solve(name)
    out, work_out, links = buffers or SC.stitch_buffers(lib, c.lag, d["count"].shape[0], c.C, c.N)
    SC.run_stitch(lib, h, d, c.L, table, work, out, work_out, links, c.lag, c.C, c.N, c.gate, c.max_gap, stream=stream)
    torch.cuda.synchronize()
    return out, work_out, links


def _bars(table):
    """``tracklog_ref.bars`` of a table; where a lane holds a NaN (nonfinite) the same figure over the finite words."""
    bars = R.bars(table.err)
    if np.isfinite(list(bars.values())).all():
        return bars
    with np.errstate(invalid="ignore"):
        return {n: 4.0 * float(np.nanmax(np.abs(getattr(table, n + "32") - getattr(table, n)))) for n in ("filt", "smooth")}


def _close(got, ref, bar, what):
    """``got`` within ``bar`` of the float64 ``ref`` where that is finite, the same NaNs elsewhere; returns the worst error."""
    finite = np.isfinite(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    err = float(np.abs(got.astype(np.float64) - ref)[finite].max()) if finite.any() else 0.0
    assert err <= bar, (what, err, bar)
    return err


@pytest.mark.parametrize("name", SC.NAMES)
def test_the_stitch_against_the_reference(name):
    c, ref = SC.make(name), SC.reference(name)
    assert ref.stitch.undecided == 0
    lib, h, d, table, work = _solve(name)
    B = d["count"].shape[0]
    inputs = list(table.items()) + list(d.items()) + [("work", work)]
    before = {k: v.clone() for k, v in inputs}
    out, work_out, links = _stitch(name)
    for k, v in inputs:
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k                  # it writes only its outputs
    assert np.array_equal(table["state"].cpu().numpy(), ref.solve.state)                         # (the kernel's solve is the reference's)
    got = {k: v.cpu().numpy() for k, v in list(out.items()) + list(links.items())}
    got["work_out"] = work_out.cpu().numpy().reshape(B, c.lag, c.C).transpose(1, 0, 2)
    for k, v in got.items():                                                                     # every word was written
        assert not (v == -7).any(), k
    s = ref.stitch
    for k in LINK_INTS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], getattr(s, k)), (k, got[k].tolist(), getattr(s, k).tolist())
    for k in INTS:
        assert np.array_equal(got[k], getattr(s.table, k)), (k, np.argwhere(got[k] != getattr(s.table, k))[:8])
    assert np.array_equal(got["work_out"], s.work_out), np.argwhere(got["work_out"] != s.work_out)[:8]
    assert np.array_equal(got["size"].view(np.uint32), s.table.size.view(np.uint32))
    d2_bar = 4.0 * s.d2_err
    d2_err = float(np.abs(got["link_d2"].astype(np.float64) - s.link_d2).max())
    same32 = bool(np.array_equal(got["link_d2"].view(np.uint32), s.link_d2_32.view(np.uint32)))
    bars = _bars(s.table)
    errs = {n: _close(got[n], getattr(s.table, n), bars[n], (name, n)) for n in ("filt", "smooth")}
    print(name, "links", s.n_links.tolist(), "d2 error of the restatement", s.d2_err, "the kernel's", d2_err, "allowed", d2_bar,
          "the restatement's bits", same32, "stitched filt / smooth errors", errs, "bars", bars)
    SC.record("cases", name, shape=dict(N=c.N, C=c.C, L=c.L, lag=c.lag, lanes=B, gate=c.gate, max_gap=c.max_gap), links=s.n_links.tolist(),
              d2=dict(restatement_error=s.d2_err, kernel_error=d2_err, allowed=d2_bar, restatement_bits=same32),
              bars=bars, kernel_error=errs)
    assert got["link_d2"].dtype == np.float32 and np.isfinite(got["link_d2"]).all()
    assert np.array_equal(got["link_d2"] == 0, s.link_d2 == 0) and d2_err <= d2_bar, (d2_err, d2_bar)


@pytest.mark.parametrize("name", SC.BITS)
def test_the_stitched_table_has_the_bits_of_the_solve_of_the_log_never_relabelled(name):
    c = SC.make(name)
    out, work_out, _ = _stitch(name)
    _, _, _, plain, plain_work = _solve(name, plain=True)
    for k in BIT_FIELDS:
        assert torch.equal(out[k].view(torch.uint8), plain[k].view(torch.uint8)), (name, k)
    assert torch.equal(work_out, plain_work), name


def test_a_replayed_graph_gives_the_eager_calls_bits():
    name = "relabel_chain"
    c = SC.make(name)
    lib, h, d, table, work = _solve(name)
    eager = _stitch(name)
    bufs = SC.stitch_buffers(lib, c.lag, d["count"].shape[0], c.C, c.N)
    tensors = lambda b: list(b[0].items()) + [("work_out", b[1])] + list(b[2].items())
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    SC.run_stitch(lib, h, d, c.L, table, work, *bufs, c.lag, c.C, c.N, c.gate, c.max_gap, stream=side)
    assert lib.sqair_capture_end(h, ss, 1) == 1, lib.sqair_last_error(h)                        # one launch: one kernel node
    torch.cuda.synchronize()
    assert all((t == -7).all() for _, t in tensors(bufs))                                       # (a capture launches nothing)
    for _ in range(2):
        for _, t in tensors(bufs):
            t.fill_(-7)
        torch.cuda.synchronize()
        assert lib.sqair_capture_launch(h, 1, ss) == 0, lib.sqair_last_error(h)
        torch.cuda.synchronize()
        for (k, t), (_, e) in zip(tensors(bufs), tensors(eager)):
            assert torch.equal(t.view(torch.uint8), e.view(torch.uint8)), k


def test_the_scorer_on_the_stitched_table_gives_the_references_counters():
    name = "dropout"
    c, ref = SC.make(name), SC.reference(name)
    lib, h, d, table, _ = _solve(name)
    out, _, _ = _stitch(name)
    truth = TC.to_device(c.truth)
    fig = {}
    for label, tab, want in (("before", table, ref.solve), ("after", out, ref.stitch.table)):
        buf = SCC.score_buffers(c.lag, 1, 1)
        SCC.run_score(lib, h, d, c.L, tab, truth, buf, c.lag, c.C, 1, 0, iou_min=SC.IOU_MIN)
        torch.cuda.synchronize()
        counts = buf["counts"].cpu().numpy()
        expect = SCR.score(SC.table_of(want), c.log["log_valid"], c.truth, SC.IOU_MIN)
        assert np.array_equal(counts, expect.counts), (label, counts.tolist(), expect.counts.tolist())
        fig[label] = dict({n: int(counts[:, FILLED, K[n]].sum()) for n in ("idsw", "gap_tp", "tp", "fn")},
                          idf1=SCR.pooled(counts, buf["sums"].cpu().numpy(), FILLED)["idf1"])
    print("dropout, smooth_filled: before", fig["before"], "after", fig["after"])
    SC.record("cases", "dropout_score", **fig)
    assert fig["after"]["idsw"] == 0 and fig["after"]["idf1"] == 1.0 and fig["after"]["gap_tp"] == 12
    assert fig["before"]["idsw"] == 1 and fig["before"]["gap_tp"] == 0
