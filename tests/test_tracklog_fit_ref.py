"""No GPU: the reference of motion calibration (tests/tracklog_fit_ref.py) on the cases of tests/tracklog_fit_cases.py, held to what
does not depend on it -- the likelihood of the dense Gaussian the model defines, built with numpy.linalg; the recovery of the
simulation's true (q, r) with a margin far above the bars; the identities between the counters; what each case is there to exercise
-- and ``lane.track_log_fit`` on hand-made sums.  The kernel is held to this reference by tests/test_tracklog_fit_kernel.py."""
import numpy as np
import pytest
import torch

from sqair_amd import lane as LN
from tests import tracklog_fit_cases as FC
from tests import tracklog_fit_ref as FR
from tests import tracklog_ref as R

NAMES = list(FC.CASES)
K = {n: i for i, n in enumerate(FR.COUNTS)}
S = {n: i for i, n in enumerate(FR.SUMS)}


def test_the_innovations_form_equals_the_dense_gaussian():
    """On ``sim``, per (lane, column, axis) and with no burn: the walk's 1/2 sum (ln 2 pi S + y^2 / S) is -log p of the later sightings
    under the Gaussian the model defines, assembled entry by entry and evaluated with numpy.linalg -- at the true node and at the
    default scalars."""
    x = FC.inputs("sim")
    lag, B, C = x.solve.state.shape
    L = x.L
    n_chains = 0
    for q, r in (FC.SIM_TRUE, (0.25, 1.0)):
        for b in range(B):
            for c in range(C):
                if x.solve.track_id[b, c] < 0:
                    continue
                one = np.zeros_like(x.solve.state)
                one[:, b, c] = x.solve.state[:, b, c]                                    # this column alone
                ref = FR.fit(x.log, x.solve.frame_index, one, x.slot, (q,), (r,), FC.V0_VAR, 0)
                stepped = [f for f in range(lag) if one[f, b, c] in (R.SEEN, R.GAP)]
                assert stepped == list(range(stepped[0], stepped[-1] + 1))            # (every frame is finite: consecutive)
                total, terms = 0.0, 0
                for ax in range(2):
                    zs = []
                    for f in stepped:
                        bx = x.log["log_box"][b, int(x.solve.frame_index[f, b] % L), x.slot[f, b, c]]
                        zs.append(0.5 * float(bx[2 + ax]) + float(bx[ax]) if one[f, b, c] == R.SEEN else None)
                    nll, m = FR.dense_nll(zs, q, r, FC.V0_VAR)
                    total, terms = total + nll, terms + m
                got = float(FR.nll(ref.counts, ref.sums)[0, 0])
                assert terms == ref.counts[b, 0, 0, K["n"]] and terms > 20
                assert abs(got - total) <= 1e-9 * abs(total), (b, c, got, total)
                n_chains += 1
    assert n_chains == 2 * B * 2


def test_the_reference_recovers_the_simulations_scalars():
    x, ref = FC.inputs("sim"), FC.reference("sim")
    nll = FR.nll(ref.counts, ref.sums)
    node = np.unravel_index(int(np.argmin(nll)), nll.shape)
    assert node == FC.SIM_NODE and (x.q_grid[node[0]], x.r_grid[node[1]]) == FC.SIM_TRUE
    second = np.unravel_index(int(np.argsort(nll.ravel())[1]), nll.shape)
    runner_up = float(nll[second] - nll[node])
    nll_bar = FR.nll_bars(ref)
    bar = float(max(nll_bar[node], nll_bar[second]))                                  # the NLL's bar at the two nodes compared
    print("terms", int(ref.counts[:, node[0], node[1], K["n"]].sum()), "margin to the runner-up", runner_up, "nats; the NLL's bar there", bar,
          "the largest over the grid", float(nll_bar.max()), "term errors at the fit", {n: float(e[node]) for n, e in ref.term_err.items()},
          "the worst over the grid", FR.worst(ref.term_err))
    assert runner_up >= 1000.0 * bar and bar > 0.0                                   # the condition: asserted, never skipped
    # and no node of the grid can change places with the minimum inside the bars: every margin is above the two nodes' bars together
    others = np.ones(nll.shape, bool)
    others[node] = False
    assert ((nll - nll[node])[others] > (nll_bar + nll_bar[node])[others]).all()
    tot = ref.counts.sum(0)
    mean_nis = ref.sums.sum(0)[..., S["nis_sum"]] / tot[..., K["n"]]
    print("mean NIS at the fit", mean_nis[node], "at the default scalars", mean_nis[4, 4])
    assert 0.9 <= mean_nis[node] <= 1.1 and mean_nis[4, 4] > mean_nis[node]
    assert tot[node][K["n_gap"]] > 0 and not tot[..., K["skipped"]].any()


@pytest.mark.parametrize("name", NAMES)
def test_the_identities_between_the_counters(name):
    x, ref = FC.inputs(name), FC.reference(name)
    c = ref.counts
    assert (c >= 0).all() and (c[..., K["n_gap"]] <= c[..., K["n"]]).all()
    expect = FR.expected_terms(x.solve.state, x.burn)
    assert (c[..., K["n"]] + c[..., K["skipped"]] == expect[:, None, None]).all()
    assert ref.undecided == 0                                                           # the restatement decides as float64 does
    assert np.isfinite(ref.sums).all() and np.isfinite(ref.sums32).all()
    assert not ref.sums[c[..., K["n"]] == 0].any() and not ref.sums[..., 2:][c[..., K["n_gap"]] == 0].any()
    assert all(np.isfinite(e).all() for e in ref.term_err.values()), ref.term_err
    later = np.zeros(x.solve.state.shape, bool)                                        # innov: nonzero exactly at the later sightings
    seen = x.solve.state == R.SEEN
    later[1:] = seen[1:] & (np.cumsum(seen, 0)[:-1] > 0)
    assert ((ref.innov[..., 1] != 0) == later[..., None]).all() and not ref.innov[~later].any()
    # the restatement's own sums lie inside a quarter of the bars (but for the rounding of the float64 additions themselves)
    assert (np.abs(ref.sums32 - ref.sums) <= FR.bars(ref) / 4.0 + 1e-12 * (1.0 + np.abs(ref.sums))).all()


def test_what_each_case_exercises():
    tot = lambda n: FC.reference(n).counts.sum((0, 1, 2))
    a = FC.inputs("a_2x2_b0")
    assert int(a.log["count"].max()) > a.L                                             # the ring wraps
    e = FC.inputs("e_2x2_b0")
    assert (e.N, e.C, e.L, e.lag) == (1, 1, 4, 4)
    f = FC.inputs("f_2x2_b0")
    assert (f.N, f.C, f.lag) == (14, 64, 16) and f.wide and (f.solve.frame_index[0] == -1).all()
    assert (FC.inputs("g_2x2_b0").solve.state == R.INVALID).any()
    assert tot("h_2x2_b0")[K["n_gap"]] > 0 and (FC.inputs("h_2x2_b0").solve.state == R.GAP).sum() >= 4
    i = FC.reference("i_2x2_b0")
    assert not i.counts.any() and not i.sums.any() and not i.innov.any() and (FC.inputs("i_2x2_b0").solve.state == R.SEEN).sum() == 1
    assert not (FC.inputs("j_2x2_b0").solve.state != 0).any() and not FC.reference("j_2x2_b0").counts.any()
    for base in "aefgh":
        assert tot(base + "_2x2_b0")[K["n"]] > tot(base + "_2x2_b2")[K["n"]] or base == "e", base    # burn drops terms
        assert FC.reference(base + "_3x1_b0").counts.shape[1:3] == (3, 1)
    p = FC.inputs("p")
    assert 256 % (2 * p.C) != 0 and len(p.q_grid) == len(p.r_grid) == 16 and (p.solve.track_id >= 0).sum(1).max() == p.C
    w = FC.inputs("w")
    assert w.C == 64 and w.solve.state.shape[:2] == (12, 2) and tot("w")[K["n"]] > 0
    l = FC.inputs("l")
    assert l.lag == 200 and l.lag > 6 * FC.BLOCK and l.lag % FC.BLOCK != 0 and l.L == 256 and l.solve.state.shape[1:] == (2, 2)
    assert tot("l")[K["n_gap"]] > 0
    bad = FC.reference("bad")
    assert tot("bad")[K["skipped"]] > 0 and tot("bad")[K["n"]] > 0 and np.isfinite(bad.sums).all() and not np.isfinite(bad.innov).all()
    s = FC.inputs("sim")
    assert s.solve.state.shape == (32, 8, 4) and (s.N, s.L, s.lag) == (2, 32, 32) and (s.solve.n_tracks == 2).all()
    frac = (s.solve.state[:, :, :2] == R.GAP).mean()
    assert 0.05 < frac < 0.25


def test_lane_track_log_fit_on_hand_made_sums():
    q_grid, r_grid = (0.5, 1.0, 2.0), (1.0, 4.0)
    counts = np.zeros((2, 3, 2, 3), np.int64)
    sums = np.zeros((2, 3, 2, 4))
    counts[0, ..., 0], counts[0, ..., 1] = 10, 2
    sums[0, ..., 0] = [[30.0, 20.0], [12.0, 10.0], [14.0, 16.0]]                      # nis_sum: node (1, 1) is lane 0's minimum
    sums[0, ..., 1] = 1.0
    sums[0, ..., 2], sums[0, ..., 3] = 4.0, 0.5
    counts[1, 0, 0] = (4, 0, 1)                                                         # lane 1: terms at node (0, 0) alone ...
    sums[1, 0, 0, :2] = (2.0, -60.0)                                                    # ... and low enough to move the pooled minimum
    got = LN.track_log_fit(dict(counts=torch.from_numpy(counts), sums=torch.from_numpy(sums)), q_grid, r_grid)
    ln2pi = np.log(2.0 * np.pi)
    assert got["lane_nll"].shape == (2, 3, 2) and got["nll"].shape == (3, 2) and got["nll"].dtype == torch.float64
    assert abs(float(got["lane_nll"][0, 1, 1]) - 0.5 * (10 * ln2pi + 1.0 + 10.0)) < 1e-12
    assert abs(float(got["nll"][0, 0]) - 0.5 * (14 * ln2pi + (1.0 - 60.0) + (30.0 + 2.0))) < 1e-12
    assert got["node"] == (0, 0) and (got["q"], got["r"]) == (0.5, 1.0) and got["at_edge"] is True
    assert got["lane_q"].tolist() == [1.0, 0.5] and got["lane_r"].tolist() == [4.0, 1.0]
    assert float(got["mean_nis"][1, 1]) == 1.0 and float(got["gap_mean_nis"][1, 1]) == 2.0 and float(got["lane_mean_nis"][1, 0, 0]) == 0.5
    assert np.isnan(float(got["lane_mean_nis"][1, 1, 1])) and np.isnan(float(got["lane_gap_mean_nis"][1, 0, 0]))
    assert got["n"].tolist() == [[14, 10], [10, 10], [10, 10]] and int(got["skipped"][0, 0]) == 1 and int(got["n_gap"][2, 1]) == 2
    assert "innov" not in got and got["q_grid"].tolist() == list(q_grid)
    # an interior minimum is not at the edge; an axis of one value does not count as a border; no term at all: no fit
    sums[1, 0, 0, 1] = 0.0
    inner = LN.track_log_fit(dict(counts=counts[:, :, 1:], sums=sums[:, :, 1:]), q_grid, r_grid[1:])
    assert inner["node"] == (1, 0) and inner["at_edge"] is False and (inner["q"], inner["r"]) == (1.0, 4.0)
    none = LN.track_log_fit(dict(counts=np.zeros((1, 3, 2, 3), np.int64), sums=np.zeros((1, 3, 2, 4)), innov=np.zeros((4, 1, 2, 2, 2))),
                            q_grid, r_grid)
    assert none["node"] is None and np.isnan(none["q"]) and np.isnan(none["r"]) and none["at_edge"] is False
    assert torch.isnan(none["lane_q"]).all() and none["innov"].shape == (4, 1, 2, 2, 2)
    with pytest.raises(ValueError, match="lane.track_log_fit"):
        LN.track_log_fit(dict(counts=counts, sums=sums), q_grid, q_grid)
