"""-m gpu: object layers inside the streaming pass (include/sqair_hip.h: sqair_set_layers; SqairStream(estimate_layers=True)), on the
configuration and batch of tests/test_estimate_stream.py (B = 4, K = 3, N = 3, 50 x 50), a dozen steps each.

Checked here: switching the layers on changes nothing else, bit for bit, and adds exactly one graph node to an estimate-only
stream; graph replay and eager steps give the same bits; ``out["lane"]``'s layers equal the float64 reference (tests/layers_ref.py)
applied to the step's own ``glimpse``, ``where``, ``presence`` and log weights -- ``match`` exactly but for decisions within 1e-5 of a
threshold (counted, at most 1 %), ``layer`` and ``cover`` within 2e-5 of the reference evaluated with the device's own match table,
``owner`` exactly the rule on the device's own cover -- without SMC and with it, at frames_per_step 1 and 3, with a coasted lane and
across reset(); the two glimpse buffers of the pass (``"glimpse"`` bound or not) give the same bits; a K = 1 stream recomposes its own
``canvas``; and the weight of the particles with a match is the estimate's ``support``."""
import numpy as np
import pytest
import torch

from tests import estimate_check as EC
from tests import layers_cases as LC
from tests import layers_ref as L
from tests.stream_harness import EST_KEYS, OUTS, SCORE, SMC_OUTS, words, cap, carried_in, host, same_bits, setup, stream

pytestmark = pytest.mark.gpu

GL_OUTS = OUTS + ("glimpse",)
LAYER_KEYS = ("match", "layer", "cover", "owner")
HW, FLAGS, B, IOU = SCORE.HW, SCORE.FLAGS, SCORE.B, SCORE.IOU
COVER_MIN = 0.5


def _setup(T, flags=FLAGS, seed=11):
    return setup(flags, B, T, HW, seed)


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=kw.pop("outputs", OUTS), **kw)


def _layers(F, P, **kw):
    return _stream(F, P, estimate=True, estimate_iou=IOU, estimate_layers=True, layers_cover_min=COVER_MIN, **kw)


def _check_step(st, o, lw0, counts):
    """out["lane"]'s layers of one step against the reference applied to the step's own per-row outputs and ``lw0``."""
    lane, K = o["lane"], st.K
    args = (o["glimpse"], o["where"], o["presence"], o["log_weights_per_timestep"], K, HW, IOU, COVER_MIN)
    ref = L.layers(*args, lw0=lw0)
    assert not ref.bad.any()
    near, decisions = L.near_decisions(ref.est, IOU)
    differ = lane["match"] != ref.match
    assert not (differ & ~near).any(), np.argwhere(differ & ~near)[:4]
    counts["decisions"] += decisions
    counts["near"] += int(near.sum())
    own = L.layers(*args, lw0=lw0, match=lane["match"])
    for name in ("layer", "cover"):
        err = np.abs(lane[name].astype(np.float64) - getattr(own, name)).max()
        counts[name] = max(counts[name], float(err))
        assert err <= LC.TOL, (name, err)
        assert not words(lane[name][~ref.present]).any(), name
    assert np.array_equal(lane["owner"], L.owner_rule(lane["cover"], ref.present, COVER_MIN))
    counts["objects"] += int(ref.present.sum())
    counts["owned"] += int((lane["owner"] >= 0).sum())
    counts["unmatched"] += int((lane["match"][np.broadcast_to(ref.present[:, :, None, :], differ.shape)] == -1).sum())
    # the weight of the particles with a match is the estimate's support: the same weights added in the same order
    terms = np.where(lane["match"] >= 0, lane["weights"][..., None].astype(np.float64), 0.0).transpose(0, 1, 3, 2)   # [T, B, N, K]
    band = np.minimum(EC._sum_band(terms, np.zeros_like(terms)), EC.CAP * terms.sum(-1)) + EC.TINY
    assert (np.abs(lane["support"].astype(np.float64) - terms.sum(-1)) <= band).all()
    return ref


def _counts():
    return dict(decisions=0, near=0, layer=0.0, cover=0.0, objects=0, owned=0, unmatched=0)


def _cap(counts):
    cap(counts, skipped="near")
    assert counts["objects"] > 0 and counts["owned"] > 0, counts


# ---- 1. nothing else changes; one node more; graph == eager; the two glimpse buffers --------------------------------------------------
def test_the_layers_change_nothing_else():
    T = 12
    F, P, obs, noise = _setup(T)
    smc = dict(resample="systematic", ess_frac=0.5, seed=5)
    off = _stream(F, P, estimate=True, estimate_iou=IOU, **smc)
    on = _layers(F, P, **smc)
    eager = _layers(F, P, use_graph=False, **smc)
    bound = _layers(F, P, outputs=GL_OUTS, **smc)       # the decoder writes the caller's glimpse buffer, not the workspace's
    went = 0
    for t in range(T):
        a, b, c, d = (host(s.step(obs[t:t + 1], noise=noise[t:t + 1])) for s in (off, on, eager, bound))
        assert set(a["lane"]) == EST_KEYS and set(b["lane"]) == EST_KEYS | set(LAYER_KEYS)
        same_bits(a, b, OUTS + SMC_OUTS, t)
        same_bits(a["lane"], b["lane"], EST_KEYS, t)
        for k in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src"):
            assert torch.equal(getattr(off, k), getattr(on, k)), (t, k)
        same_bits(b["lane"], c["lane"], b["lane"].keys(), (t, "eager"))      # eager and graph: the same bits
        same_bits(b["lane"], d["lane"], b["lane"].keys(), (t, "glimpse bound"))
        assert b["lane"]["layer"].shape == (1, B, 3) + HW and b["lane"]["owner"].shape == (1, B) + HW
        assert b["lane"]["match"].shape == (1, B, on.K, 3) and b["lane"]["match"].dtype == np.int32
        went += int(b["resampled"].sum())
    assert went > 0
    assert on.core.graph_nodes() == off.core.graph_nodes() + 1
    for s in (off, on, eager, bound):
        s.close()


# ---- 2. against the reference: without SMC, with SMC; frames_per_step 1 and 3 ------------------------------------------------------------
@pytest.mark.parametrize("resample,Ts", [(None, 1), ("systematic", 1), (None, 3), ("systematic", 3)],
                         ids=["plain", "smc", "plain_T3", "smc_T3"])
def test_layers_against_reference(resample, Ts):
    steps = 12 // Ts
    F, P, obs, noise = _setup(Ts * steps, seed=3)
    st = _layers(F, P, outputs=GL_OUTS, frames_per_step=Ts, resample=resample, ess_frac=0.5, seed=17)
    counts = _counts()
    for s in range(steps):
        lw0 = carried_in(st)
        o = host(st.step(obs[s * Ts:(s + 1) * Ts], noise=noise[s * Ts:(s + 1) * Ts]))
        _check_step(st, o, lw0, counts)
    _cap(counts)
    st.close()


# ---- 3. a coasted lane: the decoder ran on its coasted records -------------------------------------------------------------------------
def test_a_coasted_lane_needs_no_special_case():
    T = 12
    F, P, obs, noise = _setup(T, seed=13)
    st = _layers(F, P, outputs=GL_OUTS, missing=True)
    counts = _counts()
    rng = np.random.default_rng(2)
    coasted = 0
    for t in range(T):
        observed = np.ones(B, bool) if t < 2 else rng.uniform(size=B) < 0.6
        lw0 = carried_in(st)
        o = host(st.step(obs[t:t + 1], noise=noise[t:t + 1], observed=observed))
        _check_step(st, o, lw0, counts)
        coasted += int((~observed).sum())
    assert coasted > 4
    _cap(counts)
    st.close()


# ---- 4. reset: the layers follow the rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample", [None, "systematic"])
def test_layers_across_reset(resample):
    T = 12
    F, P, obs, noise = _setup(T, seed=19)
    st = _layers(F, P, outputs=GL_OUTS, resample=resample, ess_frac=0.5)
    counts = _counts()
    for t in range(T):
        if t == 4:
            st.reset([1])
        if t == 9:
            st.reset([0, 3])
        lw0 = carried_in(st)
        o = host(st.step(obs[t:t + 1], noise=noise[t:t + 1]))
        _check_step(st, o, lw0, counts)
    _cap(counts)
    st.close()


# ---- 5. K = 1: the layers recompose the pass's own canvas ---------------------------------------------------------------------------------
def test_k1_recomposes_the_streams_canvas():
    T = 12
    F, P, obs, noise = _setup(T, flags=dict(k_particles=1, n_steps_per_image=3), seed=5)
    st = _layers(F, P, outputs=OUTS + ("canvas",))
    mean_img = P["dec.mean_img"].reshape(HW).astype(np.float64)
    present = 0
    for t in range(T):
        o = host(st.step(obs[t:t + 1], noise=noise[t:t + 1]))
        lane = o["lane"]
        ms = lane["cover"].astype(np.float64).sum(2)
        got = lane["layer"].astype(np.float64).sum(2) + mean_img * (1.0 / (1.0 + np.exp(10.0 - 20.0 * ms)))
        err = np.abs(got - o["canvas"].reshape(1, B, *HW)).max()
        assert err <= LC.TOL, (t, err)
        assert np.array_equal(lane["match"][0, :, 0], np.where(lane["presence"][0] != 0, np.arange(3)[None], -1))
        present += int((lane["presence"] != 0).sum())
    assert present > 0
    st.close()
