"""-m gpu: SMC resampling inside the streaming pass (include/sqair_hip.h: sqair_set_smc; SqairStream(resample="systematic")).

The resampler kernel at the end of every pass turns each lane's log weights into ESS, the SMC evidence and the next pass's source
map.  Checked here: ess_frac = 0 changes nothing; decisions, ESS, evidence and ancestors against a float64 NumPy systematic
resampler; the same continuation as a host-driven resample(); graph replay equal to eager steps; reset under SMC; one graph node
more; and the systematic invariants over a 100-frame stream."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.stream_harness import OUTS, SMC_OUTS, accumulate, core, host, same_values, setup

pytestmark = pytest.mark.gpu

HW = (50, 50)


def _setup(flags, B, T, seed=11):
    return setup(flags, B, T, HW, seed)


def _core(F, P, options=None):
    return core(F, HW, P, options)


# ---- 1. ess_frac = 0: never resample ---------------------------------------------------------------------------------------------
def test_never_resampling_changes_nothing():
    B, T = 4, 10
    F, P, obs, noise = _setup(dict(k_particles=3, n_steps_per_image=3), B, T)
    K = int(F.k_particles)
    R = B * K
    plain = SqairStream(_core(F, P), B, outputs=OUTS)
    smc = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=0.0)
    for t in range(T):
        a = host(plain.step(obs[t:t + 1], noise=noise[t:t + 1]))
        b = host(smc.step(obs[t:t + 1], noise=noise[t:t + 1]))
        same_values(a, b, OUTS)
        assert (b["resampled"] == 0).all()
        assert np.array_equal(b["ancestors"], np.arange(R))
    # the evidence after frame T is the IWAE bound of one whole T-frame pass
    whole = _core(F, P)
    whole.bind(T, B, "all")
    with whole.on_stream():
        whole.obs.copy_(torch.as_tensor(obs))
        whole.noise.copy_(torch.as_tensor(noise).reshape(whole.noise.shape))
        whole.forward()
    torch.cuda.synchronize()
    want = whole.elbo_iwae_per_example.cpu().numpy().astype(np.float64)
    got = b["log_evidence"].astype(np.float64)
    assert np.allclose(got, want, rtol=1e-5, atol=0), (got, want)
    assert np.array_equal(smc.log_z.cpu().numpy(), np.zeros(B, np.float32))


# ---- 2. against a float64 NumPy systematic resampler -------------------------------------------------------------------------
RESAMPLER_CASES = [(dict(k_particles=K, n_steps_per_image=3), frac, caller)
                   for K in (2, 5, 16) for frac in (0.5, 1.0) for caller in (True, False)]
RESAMPLER_CASES.append((dict(k_particles=5, n_steps_per_image=3, n_what=64), 0.5, False))   # the wide library


@pytest.mark.parametrize("flags,frac,caller", RESAMPLER_CASES,
                         ids=["K{}_f{}_{}{}".format(f["k_particles"], fr, "caller" if c else "philox", "_wide" if "n_what" in f else "")
                              for f, fr, c in RESAMPLER_CASES])
def test_resampler_against_numpy(flags, frac, caller):
    B, T = 8, 6
    F, P, obs, noise = _setup(flags, B, T, seed=3)
    K = int(F.k_particles)
    core = _core(F, P)
    if "n_what" in flags:
        assert core.lib is _capi.lib(_capi.WIDE_LIB_PATH)
    st = SqairStream(core, B, outputs=OUTS, resample="systematic", ess_frac=frac, seed=17)
    rng = np.random.default_rng(5)
    checked = skipped = went = 0
    us = []
    for t in range(T):
        lw0, lz0 = st.log_weight_sum.clone(), st.log_z.clone()
        u_in = rng.uniform(size=B).astype(np.float32) if caller else None
        out = st.step(obs[t:t + 1], noise=noise[t:t + 1], uniforms=u_in)
        u, lw1, lz1 = st.u.clone(), st.log_weight_sum.clone(), st.log_z.clone()
        o = host(out)
        lw0, lz0, u, lw1, lz1 = (x.cpu().numpy() for x in (lw0, lz0, u, lw1, lz1))
        if caller:
            assert np.array_equal(u, u_in)
        else:
            assert ((u >= 0) & (u < 1)).all()
            us.append(u)
        a = accumulate(lw0, o["log_weights_per_timestep"]).reshape(B, K).astype(np.float64)
        m = a.max(1, keepdims=True)
        e = np.exp(a - m)
        S = e.sum(1)
        ess = S * S / (e * e).sum(1)
        lse = m[:, 0] + np.log(S / K)
        assert np.allclose(o["ess"], ess, rtol=1e-5, atol=0)
        assert np.allclose(o["log_evidence"], lz0 + lse, rtol=1e-5, atol=1e-5)
        for b in range(B):
            rows = slice(b * K, (b + 1) * K)
            if frac == 1.0:
                go = True
            elif abs(ess[b] - frac * K) <= 1e-4 * K:   # (a decision inside the float noise of ESS: not checked)
                go = bool(o["resampled"][b])
            else:
                go = ess[b] < frac * K
            assert o["resampled"][b] == int(go), (t, b, ess[b])
            if not go:
                assert np.array_equal(o["ancestors"][rows], np.arange(b * K, (b + 1) * K))
                assert np.array_equal(lw1[rows], a[b].astype(np.float32))
                assert lz1[b] == lz0[b]
                continue
            went += 1
            assert (lw1[rows] == 0).all()
            assert np.isclose(lz1[b], lz0[b] + lse[b], rtol=1e-5, atol=1e-5)
            c = np.cumsum(e[b])
            thr = (np.arange(K) + np.float64(u[b])) * S[b] / K
            if np.abs(c[None, :] - thr[:, None]).min() < 1e-5 * S[b]:
                skipped += 1
                continue
            checked += 1
            want = np.minimum(np.searchsorted(c, thr, side="right"), K - 1)
            assert np.array_equal(o["ancestors"][rows], b * K + want), (t, b)
    if frac * K <= 1.0:   # (ESS >= 1: K = 2 at ess_frac 0.5 never resamples)
        assert went == 0
    else:
        assert went > 0 and checked >= 4 * skipped and checked > 0, (went, checked, skipped)
    if not caller:   # Philox: one draw per lane and step, not a constant
        assert len(np.unique(np.concatenate(us))) > B


# ---- 3. the same continuation as a host-driven resample() --------------------------------------------------------------------
def test_device_resampling_equals_host_resample():
    B, T = 4, 10
    F, P, obs, noise = _setup(dict(k_particles=4, n_steps_per_image=3), B, T, seed=23)
    a = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=1.0)
    b = SqairStream(_core(F, P), B, outputs=OUTS)
    moved = False
    for t in range(T):
        oa = host(a.step(obs[t:t + 1], noise=noise[t:t + 1]))
        ob = host(b.step(obs[t:t + 1], noise=noise[t:t + 1]))
        same_values(oa, ob, OUTS)
        assert (oa["resampled"] == 1).all()
        moved |= not np.array_equal(oa["ancestors"], np.arange(B * a.K))
        b.resample(oa["ancestors"])
    assert moved


# ---- 4. graph replay == eager steps ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells,chain", [("gru", 0), ("gru", 1), ("lstm", 0)])
def test_graph_equals_eager(cells, chain):
    B, T = 8, 20
    flags = dict(k_particles=4, n_steps_per_image=3)
    if cells == "lstm":
        flags.update(time_transition="LSTM", prior_transition="LSTM")
    F, P, obs, _ = _setup(flags, B, T, seed=29)
    runs = []
    for use_graph in (False, True):
        st = SqairStream(_core(F, P, options={"slot_chain": chain}), B, outputs=OUTS, use_graph=use_graph, seed=3,
                         resample="systematic", ess_frac=0.5)
        runs.append([host(st.step(obs[t:t + 1])) for t in range(T)])
        if chain:
            st.core.check_chain()
    went = 0
    for e, g in zip(*runs):
        same_values(e, g, OUTS + SMC_OUTS)
        went += int(e["resampled"].sum())
    assert went > 0


# ---- 5. reset under SMC ------------------------------------------------------------------------------------------------------
def test_reset_composes_with_smc():
    B, T, j = 4, 5, 2
    F, P, obs, noise = _setup(dict(k_particles=3, n_steps_per_image=3), B, 2 * T, seed=31)
    K = int(F.k_particles)
    lane = slice(j * K, (j + 1) * K)
    others = np.r_[0:j * K, (j + 1) * K:B * K]
    x = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=0.5)
    y = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=0.5)
    for t in range(T):
        x.step(obs[t:t + 1], noise=noise[t:t + 1])
        y.step(obs[t:t + 1], noise=noise[t:t + 1])
    x.reset([j])
    torch.cuda.synchronize()
    assert (x._src[lane].cpu().numpy() == -1).all()
    assert (x.log_weight_sum[lane].cpu().numpy() == 0).all() and float(x.log_z[j]) == 0.0
    z = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=0.5)   # lane j's fresh start
    went = 0
    for t in range(T, 2 * T):
        ox = host(x.step(obs[t:t + 1], noise=noise[t:t + 1]))
        oy = host(y.step(obs[t:t + 1], noise=noise[t:t + 1]))
        oz = host(z.step(obs[t:t + 1], noise=noise[t:t + 1]))
        for k in OUTS:
            assert np.array_equal(ox[k][:, lane], oz[k][:, lane], equal_nan=True), k
            assert np.array_equal(ox[k][:, others], oy[k][:, others], equal_nan=True), k
        for k in ("ess", "resampled", "log_evidence"):
            assert ox[k][j] == oz[k][j], k
            assert np.array_equal(np.delete(ox[k], j), np.delete(oy[k], j)), k
        assert np.array_equal(ox["ancestors"][lane], oz["ancestors"][lane])
        assert np.array_equal(ox["ancestors"][others], oy["ancestors"][others])
        went += int(ox["resampled"].sum())
    assert went > 0
    # the reset lane is not what the lane would have been without it
    assert not np.array_equal(ox["log_weights_per_timestep"][:, lane], oy["log_weights_per_timestep"][:, lane])


# ---- 6. one node more -----------------------------------------------------------------------------------------------------------
def test_graph_has_exactly_one_node_more():
    B = 4
    F, P, obs, noise = _setup(dict(k_particles=2, n_steps_per_image=3), B, 1, seed=51)

    def nodes(**kw):
        core = _core(F, P)
        st = SqairStream(core, B, outputs=OUTS, **kw)
        st.step(obs, noise=noise)
        torch.cuda.synchronize()
        return core.graph_nodes()

    n_state = nodes()
    assert n_state > 50
    assert nodes(resample="systematic", ess_frac=0.5) == n_state + 1
    assert nodes(resample="systematic", ess_frac=0.0) == n_state + 1


# ---- 7. systematic invariants over a long stream -----------------------------------------------------------------------------
def test_systematic_invariants_on_a_long_stream():
    B, K, T, frac = 8, 5, 100, 0.5
    F, P, obs, _ = _setup(dict(k_particles=K, n_steps_per_image=3), B, T, seed=41)
    st = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=frac, seed=9)
    went = 0
    for t in range(T):
        lw0 = st.log_weight_sum.clone()
        o = host(st.step(obs[t:t + 1]))
        lw1 = st.log_weight_sum.cpu().numpy()
        a = accumulate(lw0.cpu().numpy(), o["log_weights_per_timestep"]).reshape(B, K).astype(np.float64)
        w = np.exp(a - a.max(1, keepdims=True))
        w /= w.sum(1, keepdims=True)
        assert np.array_equal(o["resampled"], (o["ess"] < np.float32(frac * K)).astype(np.int32)), t
        anc = o["ancestors"].reshape(B, K) - (np.arange(B) * K)[:, None]
        assert ((anc >= 0) & (anc < K)).all()
        assert (np.diff(anc, axis=1) >= 0).all(), t
        for b in range(B):
            if not o["resampled"][b]:
                assert np.array_equal(anc[b], np.arange(K))
                continue
            went += 1
            n = np.bincount(anc[b], minlength=K)
            assert (n >= np.floor(K * w[b] - 1e-5)).all() and (n <= np.ceil(K * w[b] + 1e-5)).all(), (t, b, n, K * w[b])
            assert (lw1[b * K:(b + 1) * K] == 0).all()
    assert went >= T // 10, went
    assert np.isfinite(o["log_evidence"]).all()
