"""-m gpu: motion calibration on a stream (SqairStream(estimate=True, identity=True, tracklog=L); ``track_log_fit()``, ``set_motion()``;
include/sqair_hip.h: sqair_lane_tracklog_fit), B = 4, K = 3 or 5, N = 3, 50 x 50, a dozen frames of make_sequences.

Checked here: ``track_log_fit()`` equals the reference fit (tests/tracklog_fit_ref.py) of the log rebuilt from the steps' own outputs
-- counters exactly, sums within the bars measured on that run, the host's figures formed from them --, with the ring wrapped, over a
shorter window, with and without ``innov``; it leaves ``track_log(lag)``'s bytes, every following step's output bits and the graph's
node count alone; single steps equal chunks of three bit for bit; ``reset([1])`` takes lane 1's earlier frames out of the fit; it works
without ``motion=True`` and composed with ``missing=True`` and SMC.  ``set_motion`` with the current values keeps every bit of the
following steps, ``set_motion(q2, r2)`` before the first step equals a stream constructed with them bit for bit, and the defaults of
``track_log()`` and ``track_log_fit()`` follow it."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import tracklog_fit_cases as FC
from tests import tracklog_fit_ref as FR
from tests import tracklog_ref as R
from tests.stream_harness import OUTS, SCORE, run, same_bits, same_bytes, setup, stream

pytestmark = pytest.mark.gpu

HW = (50, 50)
FLAGS = dict(k_particles=5, n_steps_per_image=3)
B, N, L, TRACKS = 4, 3, 8, 6
IDENT = dict(identity=True, identity_iou=0.3, identity_reid_dist=4.0, identity_max_age=3)
SCALARS = (0.25, 1.0, 16.0)
MOTION = dict(motion=True, motion_q=SCALARS[0], motion_r=SCALARS[1], motion_v0=SCALARS[2], motion_gate=3.0)
LOG = dict(tracklog=L, tracklog_tracks=TRACKS)
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)
T = 12
GRID = ((0.0625, 0.25, 1.0), (0.25, 1.0))
K = {n: i for i, n in enumerate(FR.COUNTS)}
S = {n: i for i, n in enumerate(FR.SUMS)}


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=0.5, **kw)


def _reference_log(outs, records=L, resets=None, lanes=B):
    """The reference's append of the steps' own lane outputs; ``resets``: {step: lanes} whose count is zeroed ahead of that step."""
    log = R.new_log(lanes, records, N)
    for s, o in enumerate(outs):
        for b in (resets or {}).get(s, ()):
            log["count"][b] = 0
        lane = o["lane"]
        log = R.append(log, lane["lane_id"], lane["track_len"], lane["best_row"], lane["box"])
    return log


def _flat(res):
    out = {}
    for k, v in res.items():
        if isinstance(v, dict):
            out.update({k + "." + kk: vv for kk, vv in _flat(v).items()})
        else:
            out[k] = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v if v is not None else -1)
    return out


def _check(st, outs, case, lag=None, grid=GRID, burn=0, resets=None, tracks=TRACKS, records=L, v0=SCALARS[2], **kw):
    """track_log_fit() against the reference's fit of the log rebuilt from the steps' own outputs."""
    log = _reference_log(outs, records, resets, st.B)
    lag = records if lag is None else lag
    solve = R.smooth(log, lag, tracks, *SCALARS)
    ref = FR.fit(log, solve.frame_index, solve.state, FR.slots(log, solve, lag), grid[0], grid[1], v0, burn)
    got = st.track_log_fit(lag=lag, q_grid=grid[0], r_grid=grid[1], burn=burn, innov=True, **kw)
    assert ref.undecided == 0
    counts = np.stack([got["lane_" + n].numpy() for n in FR.COUNTS], -1)
    assert counts.dtype == np.int64 and np.array_equal(counts, ref.counts), (case, np.argwhere(counts != ref.counts)[:8])
    bars = FR.bars(ref)
    pooled = FR.nll(ref.counts, ref.sums)
    nll_err = np.abs(got["nll"].numpy() - pooled)
    assert (nll_err <= FR.nll_bars(ref) + 1e-12 * np.abs(pooled)).all(), (case, nll_err, FR.nll_bars(ref))
    lane_nll = 0.5 * (ref.counts[..., 0] * np.log(2.0 * np.pi) + ref.sums[..., 1] + ref.sums[..., 0])
    lane_bar = 0.5 * (bars[..., S["nis_sum"]] + bars[..., S["lns_sum"]])
    assert (np.abs(got["lane_nll"].numpy() - lane_nll) <= lane_bar + 1e-12 * np.abs(lane_nll)).all(), case
    n = ref.counts.sum(0)[..., 0]
    with np.errstate(all="ignore"):
        want_nis = np.where(n > 0, ref.sums.sum(0)[..., 0] / n, np.nan)
    have = n > 0
    assert np.array_equal(np.isnan(got["mean_nis"].numpy()), ~have)
    assert (np.abs(got["mean_nis"].numpy() - want_nis)[have] * n[have] <= bars.sum(0)[..., S["nis_sum"]][have] + 1e-12).all(), case
    node = np.unravel_index(int(np.argmin(got["nll"].numpy())), pooled.shape)
    if n[node] > 0:
        assert got["node"] == tuple(int(i) for i in node) and (got["q"], got["r"]) == (grid[0][node[0]], grid[1][node[1]])
    else:
        assert got["node"] is None
    finite = np.isfinite(ref.innov)
    assert finite.all() and np.array_equal(got["innov"].numpy() == 0, ref.innov == 0)
    innov_err = float(np.abs(got["innov"].numpy() - ref.innov).max())
    assert innov_err <= 4.0 * ref.innov_err, (case, innov_err, ref.innov_err)
    tot = dict(zip(FR.COUNTS, ref.counts.sum((0, 1, 2)).tolist()))
    print(case, "lag", lag, tot, "term errors", FR.worst(ref.term_err), "nll error", float(nll_err.max()), "innov", innov_err)
    FC.record("stream", case, lag=lag, term_error=FR.worst(ref.term_err), nll_error=float(nll_err.max()), nll_bar=float(FR.nll_bars(ref).max()),
              innov=dict(err=innov_err, allowed=4.0 * ref.innov_err), counts=tot)
    return got, ref


# ---- 1. the fit is the reference's and moves nothing --------------------------------------------------------------------------------------
def test_the_fit_is_the_references_and_moves_no_bit():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 11)
    plain, on = _stream(F, P, **IDENT, **LOG), _stream(F, P, **IDENT, **LOG)
    empty = on.track_log_fit()                                                # before the first step: no term, no fit
    assert empty["node"] is None and not empty["n"].any() and np.isnan(empty["q"]) and tuple(empty["nll"].shape) == (8, 8)
    assert empty["q_grid"].tolist() == [0.25 * 4.0 ** k for k in range(-4, 4)] and empty["r_grid"][4] == 1.0 and "innov" not in empty
    half = T // 2
    a = run(plain, obs[:half], noise[:half])
    b = run(on, obs[:half], noise[:half])
    nodes = on.core.graph_nodes()
    want_log = _flat(plain.track_log(lag=5))
    _check(on, b, "half_way", lag=5)
    same_bytes(_flat(on.track_log(lag=5)), want_log, None, "track_log(lag) behind a fit")
    a += run(plain, obs[half:], noise[half:])
    b += run(on, obs[half:], noise[half:])
    for t, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, None, (t, "a fit between the steps"))
    assert on.core.graph_nodes() == nodes == plain.core.graph_nodes()         # nothing is registered, nothing recaptured
    for n in _capi.TRACKLOG_FIELDS:
        assert torch.equal(plain._tracklog[n].view(torch.uint8), on._tracklog[n].view(torch.uint8)), n
    got, ref = _check(on, b, "wrapped")                                       # 12 frames in a ring of 8
    assert ref.counts[..., K["n"]].sum() > 0
    _check(on, b, "burn_2", burn=2)
    same_bytes(_flat(on.track_log()), _flat(plain.track_log()), None, "track_log() behind the fits")
    part = on.track_log_fit(q_grid=GRID[0], r_grid=GRID[1], burn=0)
    assert "innov" not in part
    same_bytes({k: v for k, v in _flat(got).items() if k != "innov"}, _flat(part), None, "without innov")
    for s in (plain, on):
        s.close()


# ---- 2. single steps equal chunks of three; reset ------------------------------------------------------------------------------------------
def test_single_steps_equal_chunks_of_three():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 3)
    one, three = _stream(F, P, frames_per_step=1, **IDENT, **LOG), _stream(F, P, frames_per_step=3, **IDENT, **LOG)
    run(one, obs, noise, 1)
    outs = run(three, obs, noise, 3)
    got, _ = _check(three, outs, "chunks_of_three")
    for n in _capi.TRACKLOG_FIELDS:
        assert torch.equal(one._tracklog[n].view(torch.uint8), three._tracklog[n].view(torch.uint8)), n
    same_bytes(_flat(one.track_log_fit(q_grid=GRID[0], r_grid=GRID[1], burn=0, innov=True)), _flat(got), None, "single steps against chunks")
    one.close()
    three.close()


def test_reset_takes_the_lanes_earlier_frames_out():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 19)
    st = _stream(F, P, **IDENT, **LOG)
    resets = {7: [1]}

    def before(s):
        if s in resets:
            st.reset(resets[s])
            fit = st.track_log_fit(q_grid=GRID[0], r_grid=GRID[1], burn=0)
            assert not fit["lane_n"][1].any() and np.isnan(float(fit["lane_q"][1])) and fit["lane_n"][[0, 2, 3]].sum() > 0
    outs = run(st, obs, noise, before=before)
    got, ref = _check(st, outs, "reset", resets=resets)
    assert (ref.counts[1, ..., K["n"]] <= 2 * TRACKS * (T - 7 - 1)).all()
    st.close()


# ---- 3. without motion, with missing frames and SMC; set_motion --------------------------------------------------------------------------------
def test_composed_with_missing_and_smc_on_a_stream_without_motion():
    F, P, obs, noise = setup(SCORE.FLAGS, B, T, HW, 11)
    rng = np.random.default_rng(2)
    observed = np.stack([np.ones(B, bool) if t < 2 else rng.uniform(size=B) < 0.7 for t in range(T)])
    mk = lambda **kw: stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=0.5, missing=True, **SMC, **IDENT, **LOG, **kw)
    off, on = mk(), mk()
    assert not on.lane.motion
    half = T // 2
    a = run(off, obs[:half], noise[:half], observed=observed[:half])
    b = run(on, obs[:half], noise[:half], observed=observed[:half])
    _check(on, b, "composed_half_way")
    a += run(off, obs[half:], noise[half:], observed=observed[half:])
    b += run(on, obs[half:], noise[half:], observed=observed[half:])
    for t, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, None, (t, "composed"))
    assert on.core.graph_nodes() == off.core.graph_nodes()
    _check(on, b, "composed")
    for s in (off, on):
        s.close()


def test_set_motion_with_the_current_values_keeps_every_bit():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 19)
    plain, on = _stream(F, P, **IDENT, **MOTION, **LOG), _stream(F, P, **IDENT, **MOTION, **LOG)
    half = T // 2
    a = run(plain, obs[:half], noise[:half])
    b = run(on, obs[:half], noise[:half])
    nodes = on.core.graph_nodes()
    on.set_motion(q=SCALARS[0], r=SCALARS[1], v0=SCALARS[2], gate=3.0)         # registered again, recaptured on the next step
    assert on._graph is False
    a += run(plain, obs[half:], noise[half:])
    b += run(on, obs[half:], noise[half:])
    for t, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, None, (t, "set_motion with the current values"))
    assert on.core.graph_nodes() == nodes
    for k in plain._ident:                                                     # trk_kf among them: the filter's states are kept
        assert torch.equal(plain._ident[k].view(torch.uint8), on._ident[k].view(torch.uint8)), k
    vel = np.concatenate([o["lane"]["velocity"] for o in b])
    assert np.abs(vel).max() > 0
    for s in (plain, on):
        s.close()


def test_set_motion_before_the_first_step_equals_the_constructor_and_the_defaults_follow():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 19)
    q2, r2 = 1.0, 0.25
    built = _stream(F, P, **IDENT, **dict(MOTION, motion_q=q2, motion_r=r2), **LOG)
    late, other = _stream(F, P, **IDENT, **MOTION, **LOG), _stream(F, P, **IDENT, **MOTION, **LOG)
    late.set_motion(q2, r2)
    a, b, c = run(built, obs, noise), run(late, obs, noise), run(other, obs, noise)
    for t, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, None, (t, "set_motion against the constructor"))
    for k in built._ident:
        assert torch.equal(built._ident[k].view(torch.uint8), late._ident[k].view(torch.uint8)), k
    va, vc = (np.concatenate([o["lane"]["velocity"] for o in outs]) for outs in (a, c))
    assert not np.array_equal(va, vc)                                          # (the scalars do reach the kernel)
    assert late.lane.motion_scalars == built.lane.motion_scalars == dict(q=q2, r=r2, v0_var=SCALARS[2], gate=3.0)
    same_bytes(_flat(late.track_log()), _flat(built.track_log()), None, "track_log()'s defaults")
    same_bytes(_flat(late.track_log()), _flat(late.track_log(q=q2, r=r2, v0=SCALARS[2])), None, "the defaults are the new scalars")
    fit = late.track_log_fit()
    assert float(fit["q_grid"][4]) == q2 and float(fit["r_grid"][4]) == r2 and tuple(fit["nll"].shape) == (8, 8)
    same_bytes(_flat(fit), _flat(built.track_log_fit()), None, "track_log_fit()'s defaults")
    # on a stream without motion only the defaults change: no recapture, the steps' bits stay
    off = _stream(F, P, **IDENT, **LOG)
    d = run(off, obs[:2], noise[:2])
    off.set_motion(q2, r2)
    assert off._graph is True and off.lane.motion_scalars["q"] == q2
    same_bytes(_flat(off.track_log()), _flat(off.track_log(q=q2, r=r2)), None, "defaults without motion")
    for s in (built, late, other, off):
        s.close()
