"""-m gpu: lane estimates inside the streaming pass (include/sqair_hip.h: sqair_set_estimate; SqairStream(estimate=True)), on the small
configuration and batch of tests/test_smc_stream.py, a dozen steps each.

Checked here: switching the estimate on changes nothing else, bit for bit, and adds exactly one graph node; graph replay and eager
steps give the same estimate bits; ``out["lane"]`` equals the float64 reference (tests/estimate_ref.py, compared by
tests/estimate_check.py with its tolerances) applied to the step's own per-row outputs and the log weights the rows carried into the
step -- without SMC and with it, at frames_per_step 1 and 3, with missing frames, across reset() and resample(), and for the
posterior mean reconstruction."""
import numpy as np
import pytest
import torch

from tests import estimate_check as EC
from tests import estimate_ref as E
from tests.stream_harness import EST_KEYS, OUTS, SCORE, SMC_OUTS, cap, carried_in, host, same_bits, same_values, setup, stream

pytestmark = pytest.mark.gpu

HW, FLAGS, B, IOU = SCORE.HW, SCORE.FLAGS, SCORE.B, SCORE.IOU


def _setup(T, flags=FLAGS, seed=11):
    return setup(flags, B, T, HW, seed)


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=kw.pop("outputs", OUTS), **kw)


def _check_step(st, o, lw0, counts, canvas=False):
    """out["lane"] of one step against the reference applied to the step's own per-row outputs and ``lw0``."""
    ref = E.estimate(o["where"], o["presence"], o["obj_id"], o["log_weights_per_timestep"], st.K, HW, IOU, lw0=lw0, what=o["what"],
                     canvas=o["canvas"] if canvas else None)
    EC.check(o["lane"], ref, o["where"], o["presence"], st.K, HW, IOU, canvas=o["canvas"] if canvas else None, counts=counts)
    assert ("mean_canvas" in o["lane"]) == canvas
    return ref


def _cap(counts):
    cap(counts)
    assert counts["agreeing"] > 0


# ---- 1. nothing else changes; one node more; graph == eager ---------------------------------------------------------------------
def test_the_estimate_changes_nothing_else():
    T = 12
    F, P, obs, noise = _setup(T)
    smc = dict(resample="systematic", ess_frac=0.5, seed=5)
    off = _stream(F, P, **smc)
    on = _stream(F, P, estimate=True, estimate_iou=IOU, **smc)
    eager = _stream(F, P, estimate=True, estimate_iou=IOU, use_graph=False, **smc)
    went = 0
    for t in range(T):
        a, b, c = (host(s.step(obs[t:t + 1], noise=noise[t:t + 1])) for s in (off, on, eager))
        assert "lane" not in a
        same_values(a, b, OUTS + SMC_OUTS, t)
        for k in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src"):
            assert torch.equal(getattr(off, k), getattr(on, k)), (t, k)
        same_bits(b["lane"], c["lane"], b["lane"].keys(), t)    # eager and graph: the same bits
        went += int(b["resampled"].sum())
    assert went > 0
    assert on.core.graph_nodes() == off.core.graph_nodes() + 1
    for s in (off, on, eager):
        s.close()


# ---- 2. against the reference: without SMC, adaptive SMC, SMC at every step --------------------------------------------------------
@pytest.mark.parametrize("resample,frac", [(None, 0.5), ("systematic", 0.5), ("systematic", 1.0)], ids=["plain", "smc_0.5", "smc_1"])
def test_lane_estimate_against_reference(resample, frac):
    T = 12
    F, P, obs, noise = _setup(T, seed=3)
    st = _stream(F, P, estimate=True, estimate_iou=IOU, resample=resample, ess_frac=frac, seed=17)
    counts = EC.new_counts()
    for t in range(T):
        lw0 = carried_in(st)
        o = host(st.step(obs[t:t + 1], noise=noise[t:t + 1]))
        assert set(o["lane"]) == EST_KEYS
        assert o["lane"]["weights"].shape == (1, B, st.K) and o["lane"]["box"].shape == (1, B, 3, 4)
        _check_step(st, o, lw0, counts)
        if resample is not None:    # the resampler's ESS of the same rows, bit for bit
            assert np.array_equal(o["lane"]["ess"][-1].view(np.uint32), o["ess"].view(np.uint32)), (t, o["lane"]["ess"], o["ess"])
            if frac == 1.0 and t > 0:
                assert (lw0 == 0).all()       # the weights are this step's alone
    _cap(counts)
    st.close()


# ---- 3. frames_per_step = 3: frame t of a step uses the prefix weights ---------------------------------------------------------------
@pytest.mark.parametrize("resample", [None, "systematic"])
def test_frames_per_step_uses_prefix_weights(resample):
    Ts, steps = 3, 4
    F, P, obs, noise = _setup(Ts * steps, seed=7)
    st = _stream(F, P, frames_per_step=Ts, estimate=True, estimate_iou=IOU, resample=resample, ess_frac=0.5)
    counts = EC.new_counts()
    differ = False
    for s in range(steps):
        lw0 = carried_in(st)
        o = host(st.step(obs[s * Ts:(s + 1) * Ts], noise=noise[s * Ts:(s + 1) * Ts]))
        ref = _check_step(st, o, lw0, counts)
        # the reference's frame t accumulates frames 0..t only: the estimate of frame 0 is that of a one-frame step
        one = E.estimate(o["where"][:1], o["presence"][:1], o["obj_id"][:1], o["log_weights_per_timestep"][:1], st.K, HW, IOU, lw0=lw0)
        assert np.array_equal(ref.weights[0], one.weights[0]) and np.array_equal(ref.best_row[0], one.best_row[0])
        differ |= not np.array_equal(o["lane"]["weights"][0], o["lane"]["weights"][Ts - 1])
        if resample is not None:
            assert np.array_equal(o["lane"]["ess"][Ts - 1].view(np.uint32), o["ess"].view(np.uint32))
    assert differ
    _cap(counts)
    st.close()


# ---- 4. missing frames: a coasted lane keeps its weights and reports the coasted objects ----------------------------------------------
def test_a_coasted_lane_keeps_its_weights():
    T = 12
    F, P, obs, noise = _setup(T, seed=13)
    st = _stream(F, P, estimate=True, estimate_iou=IOU, missing=True)
    counts = EC.new_counts()
    rng = np.random.default_rng(2)
    prev = None
    coasted = 0
    for t in range(T):
        observed = np.ones(B, bool) if t < 2 else rng.uniform(size=B) < 0.6
        lw0 = carried_in(st)
        o = host(st.step(obs[t:t + 1], noise=noise[t:t + 1], observed=observed))
        _check_step(st, o, lw0, counts)       # (the per-row outputs of a coasted lane ARE the coasted records)
        for b in np.flatnonzero(~observed):
            coasted += 1
            assert (o["log_weights_per_timestep"][0, b * st.K:(b + 1) * st.K] == 0).all()
            for k in ("weights", "ess", "best_row"):
                assert np.array_equal(o["lane"][k][0, b], prev["lane"][k][0, b]), (t, b, k)
        prev = o
    assert coasted > 4
    _cap(counts)
    st.close()


# ---- 5. reset and resample: the estimate follows the rows ---------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [None, "systematic"])
def test_estimates_follow_reset_and_resample(resample):
    T = 12
    F, P, obs, noise = _setup(T, seed=19)
    st = _stream(F, P, estimate=True, estimate_iou=IOU, resample=resample, ess_frac=0.5)
    K, R = st.K, B * st.K
    counts = EC.new_counts()
    rng = np.random.default_rng(4)
    for t in range(T):
        if t == 4:
            st.reset([1])
        if t == 7:      # the caller's own map: lane 0 collapses onto one particle, lane 2 is shuffled, one row of lane 3 starts fresh
            src = np.arange(R)
            src[0:K] = 1
            src[2 * K:3 * K] = 2 * K + rng.permutation(K)
            src[3 * K] = -1
            st.resample(src)
        if t == 9:
            st.reset([0, 3])
            st.resample(np.arange(R)[::-1].reshape(B, K)[::-1].reshape(-1))    # every lane reversed, on top of the reset
        lw0 = carried_in(st)
        if t == 4:
            assert (lw0[K:2 * K] == 0).all()
        o = host(st.step(obs[t:t + 1], noise=noise[t:t + 1]))
        _check_step(st, o, lw0, counts)
    _cap(counts)
    st.close()


# ---- 6. the posterior mean reconstruction -------------------------------------------------------------------------------------------
def test_mean_canvas_is_the_weighted_mean_of_the_steps_canvases():
    Ts, steps = 2, 4
    F, P, obs, noise = _setup(Ts * steps, seed=23)
    st = _stream(F, P, frames_per_step=Ts, estimate=True, estimate_iou=IOU, estimate_canvas=True)
    assert "canvas" in st.outputs
    counts = EC.new_counts()
    for s in range(steps):
        lw0 = carried_in(st)
        o = host(st.step(obs[s * Ts:(s + 1) * Ts], noise=noise[s * Ts:(s + 1) * Ts]))
        assert o["lane"]["mean_canvas"].shape == (Ts, B) + HW
        _check_step(st, o, lw0, counts, canvas=True)
        # and directly: sum_k w_k canvas_k of the step's own canvases and the weights it reported, at the weights' band (1e-5 of
        # the sum of the terms' magnitudes: a decoder's canvas may be negative)
        w = o["lane"]["weights"].astype(np.float64)
        cv = o["canvas"].reshape(Ts, B, st.K, -1).astype(np.float64)
        mean, size = np.einsum("tbk,tbkp->tbp", w, cv), np.einsum("tbk,tbkp->tbp", w, np.abs(cv))
        assert (np.abs(o["lane"]["mean_canvas"].reshape(Ts, B, -1) - mean) <= 1e-5 * size + 1e-30).all()
        assert o["lane"]["mean_canvas"].std() > 0
    _cap(counts)
    st.close()
