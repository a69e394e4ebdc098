"""-m gpu: k_lane_tracklog_score through sqair_lane_tracklog_score on caller tensors, fed the kernel's OWN solve outputs
(k_lane_tracklog_smooth on the case's log), against the reference of tests/tracklog_score_ref.py run on those same outputs read back
-- the cases of tests/tracklog_score_cases.py, at most 8 lanes of 16 frames; what each exercises is listed there.

Every integer output is exact in every case and for both matchings: ``counts`` [B, 4, 14], ``match`` [4, lag, B, G]; ``match_iou``
within four times the fp32 IoU's measured error; ``assign`` is judged as ``idf_ref.check_assign`` judges -- the optimum (idtp) is
exact, the assignment one-to-one over overlapping pairs and of that weight: optimal assignments tie.  ``sums`` are held to float64
within a bar that is MEASURED -- per case four times the worst error of a term of the fp32 restatement of the header against float64,
times the sum's number of terms (tests/tracklog_score_ref.py: ``bars``), never anything the kernel gave.  No (lane, view) is fragile
on the kernel's own table either (asserted, not skipped).  A captured graph replayed twice gives the eager call's bits, the call
writes nothing but ``score``, and the moving drop-out's figures -- four misses become four hits -- come out of the kernel.  With
SQAIR_PARITY_DIR set the bars and the kernel's own error go into tracklog_score_parity.json there (the copy under profiles/ is such
a file)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import score_ref
from tests import tracklog_cases as TC
from tests import tracklog_score_cases as SC
from tests import tracklog_score_ref as SR

pytestmark = pytest.mark.gpu

NAMES = list(SC.CASES)
MODES = ("greedy", "optimal")
K = {n: i for i, n in enumerate(SR.COUNTS)}
S = {n: i for i, n in enumerate(SR.SUMS)}
_solved = {}


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _solve(name):
    """(lib, h, the device log, the kernel's solve of it on the device, the device truth), once per case."""
    if name not in _solved:
        x = SC.inputs(name)
        lib, h = TC.handle(x.N, x.wide)
        d = TC.to_device(x.log)
        out, work = TC.solve_buffers(lib, x.lag, d["count"].shape[0], x.C, x.N)
        TC.run_smooth(lib, h, d, x.L, x.lag, x.C, x.N, out, work)
        torch.cuda.synchronize()
        _solved[name] = lib, h, d, out, TC.to_device(x.truth)
    return _solved[name]


def _score(name, mode, stream=None, out=None):
    x = SC.inputs(name)
    lib, h, d, table, truth = _solve(name)
    G = SC.CASES[name].G
    out = SC.score_buffers(x.lag, d["count"].shape[0], G) if out is None else out
    SC.run_score(lib, h, d, x.L, table, truth, out, x.lag, x.C, G, MODES.index(mode), stream=stream)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_the_score_against_the_reference(name, mode):
    x = SC.inputs(name)
    lib, h, d, table, truth = _solve(name)
    before = {k: v.clone() for k, v in list(table.items()) + list(d.items()) + list(truth.items())}
    got = {k: v.cpu().numpy() for k, v in _score(name, mode).items()}
    for k, v in list(table.items()) + list(d.items()) + list(truth.items()):
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k                  # it writes only `score`
    host_table = {k: table[k].cpu().numpy() for k in SR.TABLE}
    ref = SR.score(host_table, x.log["log_valid"], x.truth, SC.IOU_MIN, mode)
    assert SR.fragile(ref, x.truth, SC.IOU_MIN) == []                                            # the condition holds on this table too
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], ref.counts), np.argwhere(got["counts"] != ref.counts)[:8]
    assert got["match"].dtype == np.int32 and np.array_equal(got["match"], ref.match), np.argwhere(got["match"] != ref.match)[:8]
    iou_tol = 4.0 * max(score_ref.iou32_error(x.truth["truth_box"], SR.view_boxes(host_table, v)[0]) for v in range(4))
    iou_err = float(np.abs(got["match_iou"] - ref.match_iou).max())
    assert got["match_iou"].dtype == np.float32 and iou_tol < 1e-5 and iou_err <= iou_tol, (iou_err, iou_tol)
    assert got["assign"].dtype == np.int32
    for b in range(ref.ov.shape[0]):
        for v in range(4):
            SR.check_assign(ref.ov[b, v], got["assign"][v, b], int(ref.counts[b, v, K["idtp"]]))
    bars = SR.bars(ref)
    err = np.abs(got["sums"] - ref.sums)
    worst = {n: float(err[..., i].max()) for n, i in S.items()}
    same32 = bool(np.array_equal(_bytes(got["sums"]), _bytes(ref.sums32)))
    print(name, mode, "term errors of the restatement", ref.term_err, "the kernel's worst error per sum", worst, "the restatement's bits", same32)
    tot = dict(zip(SR.COUNTS, ref.counts.sum(0)[3].tolist()))                                     # (smooth_filled, over the lanes)
    SC.record("cases", name + "_" + mode, shape=dict(N=x.N, C=x.C, L=x.L, lag=x.lag, G=SC.CASES[name].G, lanes=int(ref.counts.shape[0])),
              term_error=ref.term_err, kernel_error=worst, bars={n: float(bars[..., i].max()) for n, i in S.items()},
              match_iou=dict(err=iou_err, allowed=iou_tol), restatement_bits=same32, counts=tot)
    assert got["sums"].dtype == np.float64 and np.isfinite(got["sums"]).all()
    assert (err <= bars).all(), (np.argwhere(err > bars)[:8], worst, ref.term_err)


def test_greedy_and_optimal_differ_where_the_table_says_so():
    g, o = (_score("x", m)["counts"].cpu().numpy() for m in MODES)
    lag = SC.X_SHAPE["lag"]
    assert g[0, :, K["tp"]].tolist() == [lag] * 4 and o[0, :, K["tp"]].tolist() == [2 * lag] * 4
    assert np.array_equal(g[1:], o[1:])


def test_a_replayed_graph_gives_the_eager_calls_bits():
    name, mode = "a", "optimal"
    x = SC.inputs(name)
    lib, h, d, table, truth = _solve(name)
    eager = _score(name, mode)
    out = SC.score_buffers(x.lag, d["count"].shape[0], SC.CASES[name].G)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    SC.run_score(lib, h, d, x.L, table, truth, out, x.lag, x.C, SC.CASES[name].G, MODES.index(mode), stream=side)
    assert lib.sqair_capture_end(h, ss, 1) == 1, lib.sqair_last_error(h)                        # one launch: one kernel node
    torch.cuda.synchronize()
    assert all((t == -7).all() for t in out.values())                                           # (a capture launches nothing)
    for _ in range(2):
        for t in out.values():
            t.fill_(-7)
        torch.cuda.synchronize()
        assert lib.sqair_capture_launch(h, 1, ss) == 0, lib.sqair_last_error(h)
        torch.cuda.synchronize()
        for k, t in out.items():
            assert torch.equal(t.view(torch.uint8), eager[k].view(torch.uint8)), k


def test_the_optional_outputs_may_be_null():
    name = "d"
    x = SC.inputs(name)
    full = _score(name, "greedy")
    part = SC.score_buffers(x.lag, full["counts"].shape[0], SC.CASES[name].G)
    lib, h, d, table, truth = _solve(name)
    from sqair_amd import _capi
    tab = _capi.SqairTrackLogOut(**{n: table[n].data_ptr() for n in _capi.TRACKLOG_SCORE_TABLE})
    tr = _capi.SqairTrackLogTruth(G=SC.CASES[name].G, **{n: truth[n].data_ptr() for n in _capi.TRACKLOG_TRUTH_FIELDS})
    sc = _capi.SqairTrackLogScore(iou_min=SC.IOU_MIN, counts=part["counts"].data_ptr(), sums=part["sums"].data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sqair_lane_tracklog_score(h, C.byref(TC.log_struct(d, x.L)), C.byref(tab), C.byref(tr), C.byref(sc), x.lag, x.C,
                                         full["counts"].shape[0], 0, s) == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    assert torch.equal(part["counts"], full["counts"]) and torch.equal(part["sums"].view(torch.int64), full["sums"].view(torch.int64))
    assert all((part[k] == -7).all() for k in ("assign", "match", "match_iou"))


def test_the_moving_drop_out_out_of_the_kernel():
    """Gap filling moves four misses to four hits in the kernel's own counters; the smoother is within the README's 0.02 px."""
    got = {k: v.cpu().numpy() for k, v in _score("h", "greedy").items()}
    c, s = got["counts"][0], got["sums"][0]
    gap = [5, 6, 7, 8]
    for v in (0, 1):
        assert c[v, K["fn"]] == 4 and c[v, K["tp"]] == 7 and (got["match"][v, gap, 0, 0] == -1).all()
    assert c[3, K["fn"]] == 0 and c[3, K["gap_tp"]] == 4 and c[3, K["gap_fp"]] == 0 and c[3, K["tp"]] == 11
    assert c[2, K["fn"]] == 0 and c[2, K["gap_tp"]] == 4
    gap_err = {v: s[v, S["gap_err_sum"]] / c[v, K["gap_tp"]] for v in (2, 3)}
    print("gap_err", gap_err, "gap_nees", {v: s[v, S["gap_nees_sum"]] / c[v, K["gap_nees_n"]] for v in (2, 3)})
    assert gap_err[3] <= 0.02 and gap_err[2] > gap_err[3]
