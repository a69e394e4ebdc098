"""-m gpu: k_lane_tracklog_fit through sqair_lane_tracklog_fit on caller tensors, fed the kernel's OWN solve outputs
(k_lane_tracklog_smooth on the case's log: its table and its ``work``), against the reference of tests/tracklog_fit_ref.py run on
those same outputs read back -- the cases of tests/tracklog_fit_cases.py; what each exercises is listed there.

``counts`` [B, Q, R, 3] is exact in every case, and so is the zero pattern of ``innov``; ``sums`` are held to float64 within a bar that
is MEASURED -- per case and grid node four times the worst error of a term of the fp32 restatement of the header against float64,
times the sum's number of terms (tests/tracklog_fit_ref.py: ``bars``), never anything the kernel gave --; ``innov`` within four times
the restatement's error.  Every output is prefilled with -7, so every word must be written.  The call writes nothing but its outputs,
a captured graph replayed twice gives the eager call's bits, ``innov`` may be NULL, and on the simulation the argmin over the
kernel's own sums is the true node.  With SQAIR_PARITY_DIR set the bars and the kernel's own error go into
tracklog_fit_parity.json there (the copy under profiles/ is such a file)."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import lane as LN
from tests import tracklog_cases as TC
from tests import tracklog_fit_cases as FC
from tests import tracklog_fit_ref as FR

pytestmark = pytest.mark.gpu

NAMES = list(FC.CASES)
K = {n: i for i, n in enumerate(FR.COUNTS)}
S = {n: i for i, n in enumerate(FR.SUMS)}
_solved = {}


def _solve(name):
    """(lib, h, the device log, the kernel's solve of it on the device: table and work), once per log."""
    x = FC.inputs(name)
    key = FC.CASES[name].base
    if key not in _solved:
        lib, h = TC.handle(x.N, x.wide)
        d = TC.to_device(x.log)
        out, work = TC.solve_buffers(lib, x.lag, d["count"].shape[0], x.C, x.N)
        TC.run_smooth(lib, h, d, x.L, x.lag, x.C, x.N, out, work)
        torch.cuda.synchronize()
        _solved[key] = lib, h, d, out, work
    return _solved[key]


def _fit(name, stream=None, out=None, innov=True):
    x = FC.inputs(name)
    lib, h, d, table, work = _solve(name)
    out = FC.fit_buffers(x.lag, d["count"].shape[0], x.C, len(x.q_grid), len(x.r_grid)) if out is None else out
    FC.run_fit(lib, h, d, x.L, table, work, out, x.lag, x.C, x.N, x.q_grid, x.r_grid, x.burn, stream=stream, innov=innov)
    torch.cuda.synchronize()
    return out


def _reference(name):
    """The reference's fit on the kernel's own solve outputs read back."""
    x = FC.inputs(name)
    _, _, d, table, work = _solve(name)
    B = d["count"].shape[0]
    slot = work.cpu().numpy().reshape(B, x.lag, x.C).transpose(1, 0, 2)
    return FR.fit(x.log, table["frame_index"].cpu().numpy(), table["state"].cpu().numpy(), slot, x.q_grid, x.r_grid, FC.V0_VAR, x.burn)


@pytest.mark.parametrize("name", NAMES)
def test_the_fit_against_the_reference(name):
    x = FC.inputs(name)
    lib, h, d, table, work = _solve(name)
    inputs = list(table.items()) + list(d.items()) + [("work", work)]
    before = {k: v.clone() for k, v in inputs}
    got = {k: v.cpu().numpy() for k, v in _fit(name).items()}
    for k, v in inputs:
        assert torch.equal(v.view(torch.uint8), before[k].view(torch.uint8)), k                  # it writes only its outputs
    assert np.array_equal(table["state"].cpu().numpy(), x.solve.state)                           # (the kernel's solve is the reference's)
    ref = _reference(name)
    assert ref.undecided == 0
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], ref.counts), np.argwhere(got["counts"] != ref.counts)[:8]
    bars = FR.bars(ref)
    err = np.abs(got["sums"] - ref.sums)
    worst = {n: float(err[..., i].max()) for n, i in S.items()}
    same32 = bool(np.array_equal(got["sums"].view(np.uint8), ref.sums32.view(np.uint8)))
    finite = np.isfinite(ref.innov)
    assert got["innov"].dtype == np.float32 and np.array_equal(np.isnan(got["innov"]), np.isnan(ref.innov))
    assert np.array_equal(got["innov"][~finite & ~np.isnan(ref.innov)], ref.innov[~finite & ~np.isnan(ref.innov)])   # (infinities, by sign)
    with np.errstate(invalid="ignore"):   # (bad's infinities: left out by the mask)
        innov_err = float(np.abs(got["innov"].astype(np.float64) - ref.innov)[finite].max())
    innov_bar = 4.0 * ref.innov_err
    tot = dict(zip(FR.COUNTS, ref.counts.sum((0, 1, 2)).tolist()))
    print(name, "term errors of the restatement", FR.worst(ref.term_err), "the kernel's worst error per sum", worst, "the restatement's bits",
          same32, "innov", innov_err, "allowed", innov_bar)
    FC.record("cases", name, shape=dict(N=x.N, C=x.C, L=x.L, lag=x.lag, Q=len(x.q_grid), R=len(x.r_grid), burn=x.burn,
                                        lanes=int(ref.counts.shape[0])),
              term_error=FR.worst(ref.term_err), kernel_error=worst, bars={n: float(bars[..., i].max()) for n, i in S.items()},
              innov=dict(err=innov_err, allowed=innov_bar), restatement_bits=same32, counts=tot)
    assert got["sums"].dtype == np.float64 and np.isfinite(got["sums"]).all()
    assert (err <= bars).all(), (np.argwhere(err > bars)[:8], worst, FR.worst(ref.term_err))
    assert np.array_equal(got["innov"] == 0, ref.innov == 0), np.argwhere((got["innov"] == 0) != (ref.innov == 0))[:8]
    assert innov_err <= innov_bar, (innov_err, innov_bar)


def test_the_kernels_sums_recover_the_simulations_scalars():
    x = FC.inputs("sim")
    got = {k: v.cpu() for k, v in _fit("sim").items()}
    res = LN.track_log_fit(got, x.q_grid, x.r_grid)
    print("nll at the fit", float(res["nll"][res["node"]]), "mean NIS", float(res["mean_nis"][res["node"]]), "at the default scalars",
          float(res["mean_nis"][4, 4]), "gap mean NIS", float(res["gap_mean_nis"][res["node"]]))
    assert res["node"] == FC.SIM_NODE and (res["q"], res["r"]) == FC.SIM_TRUE and res["at_edge"] is False
    assert 0.9 <= float(res["mean_nis"][res["node"]]) <= 1.1
    assert float(res["mean_nis"][4, 4]) > float(res["mean_nis"][res["node"]])
    assert tuple(res["innov"].shape) == (x.lag, 8, x.C, 2, 2) and int(res["skipped"].sum()) == 0


def test_a_replayed_graph_gives_the_eager_calls_bits():
    name = "a_2x2_b2"
    x = FC.inputs(name)
    lib, h, d, table, work = _solve(name)
    eager = _fit(name)
    out = FC.fit_buffers(x.lag, d["count"].shape[0], x.C, len(x.q_grid), len(x.r_grid))
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    FC.run_fit(lib, h, d, x.L, table, work, out, x.lag, x.C, x.N, x.q_grid, x.r_grid, x.burn, stream=side)
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


def test_innov_may_be_null():
    name = "h_2x2_b0"
    full = _fit(name)
    part = _fit(name, innov=False)
    assert torch.equal(part["counts"], full["counts"]) and torch.equal(part["sums"].view(torch.int64), full["sums"].view(torch.int64))
    assert (part["innov"] == -7).all() and not (full["innov"] == -7).any()
