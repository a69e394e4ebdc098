"""-m gpu: forecasting from a stream state (include/sqair_hip.h: sqair_forecast; SqairStream.forecast).

Against the fp64 rollout of tests/forecast_ref.py started from the oracle's state after the same frames, against the whole-pass
generation mode (sample_from_prior, generate_after) it restates, and for what it must not do: a stream that forecasts between its
steps steps exactly as one that does not.  Also the source map it starts from, the predictive summaries and graph capture."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import Model, SqairCore
from sqair_amd.stream import SqairStream
from tests.forecast_ref import forecast_ref, prior_margin
from tests.hip_util import MARGIN, draw_noise, params32
from tests.stream_cases import DRAWS, EXACT, ORACLE_GATE as GATE, rollout_case
from tests.stream_harness import core as make_core, frames as _frames, host, scaled, setup

pytestmark = pytest.mark.gpu

GEN_GATE = 2e-5    # HIP against HIP: the decoder's dense kernel may differ with the row count
LSTM = dict(time_transition="LSTM", prior_transition="LSTM")

# name: (flags, frame size, B, streamed frames S, forecast frames F)
CASES = {
    "gru": (dict(k_particles=3, n_steps_per_image=3), (32, 40), 3, 4, 6),
    "lstm": (dict(k_particles=3, n_steps_per_image=2, **LSTM), (32, 40), 2, 4, 6),
    "vanilla": (dict(k_particles=3, n_steps_per_image=2, time_transition="VanillaRNN", prior_transition="VanillaRNN"), (32, 40), 2, 4, 6),
    "rw": (dict(k_particles=3, n_steps_per_image=3, prop_prior_type="rw"), (32, 40), 2, 4, 6),
    "guided": (dict(k_particles=3, n_steps_per_image=3, prop_prior_type="guided", rec_where_prior=True), (32, 40), 2, 4, 6),
    "padded_n_units": (dict(k_particles=2, n_steps_per_image=3, n_units=5), (32, 40), 2, 4, 6),
    "wide_n_what_64": (dict(k_particles=2, n_steps_per_image=3, n_what=64), (32, 40), 2, 4, 6),
    "k1": (dict(k_particles=1, n_steps_per_image=3), (32, 40), 4, 4, 6),
    "k65": (dict(k_particles=65, n_steps_per_image=1), (32, 40), 1, 3, 4),
    "frame_128": (dict(k_particles=2, n_steps_per_image=3), (128, 128), 2, 3, 4),
    "frame_below_glimpse": (dict(k_particles=2, n_steps_per_image=2), (12, 16), 2, 4, 6),
}


def _setup(flags, hw, B, T, seed=19):
    F, P, obs, _ = setup(flags, B, T, hw, seed, obs=_frames(hw, B, T, seed))
    return F, P, obs, make_core(F, hw, P)


@pytest.mark.parametrize("case", sorted(CASES))
def test_forecast_matches_the_fp64_rollout(case):
    rollout_case(case, *CASES[case])


@pytest.mark.parametrize("prior", ["rnn", "rw", "guided"])
def test_forecast_is_the_generation_mode(prior):
    """A whole pass with sample_from_prior, generate_after = t0 over T frames, against a stream over frames 0..t0 and a forecast of the
    remaining frames with the pass's own generation draws: the same kernels' bits (k_generate_prop / k_forecast_step share their
    sampling helpers).  rw / guided: the first generated frame only (the pass's later frames read the posterior logit)."""
    T, t0, B, hw = 6, 2, 3, (32, 40)
    flags = dict(k_particles=3, n_steps_per_image=3, prop_prior_type=prior, rec_where_prior=(prior != "rw"))
    Fg = make_flags(sample_from_prior=True, generate_after=t0, **flags)
    K, N, nzw = 3, 3, 4 + int(Fg.n_what) + 1
    obs = _frames(hw, B, T, 13)
    P = params32(Fg, hw, 6, 0.05, obs.mean((0, 1)))
    rng = np.random.default_rng(5)
    noise, gen = draw_noise(rng, T, B * K, N, nzw), draw_noise(rng, T, B * K, N, nzw)
    gen[..., 0, :, -1] *= 0.4   # (objects that live on for a few generated frames)
    cg = SqairCore(Fg, hw)
    cg.set_params(P)
    m = Model(obs, None, cg, K)
    m.run(noise=noise, gen_noise=gen)
    _, _, _, core = _setup(flags, hw, B, t0 + 1)
    core.set_params(P)
    st = SqairStream(core, B, frames_per_step=t0 + 1, use_graph=False)
    st.step(obs[:t0 + 1], noise=noise[:t0 + 1])
    got = host(st.forecast(T - t0 - 1, noise=gen[t0 + 1:]))
    torch.cuda.synchronize()
    frames = T - t0 - 1 if prior == "rnn" else 1
    present = 0
    for f in range(frames):
        t = t0 + 1 + f
        want = {k: getattr(m, k)[t].cpu().numpy() for k in ("presence", "obj_id", "what", "where", "canvas")}
        for k in EXACT:
            assert np.array_equal(got[k][f], want[k]), (f, k)
        live = want["presence"] > 0
        present += int(live.sum())
        for k in ("what", "where"):
            assert scaled(got[k][f][live], want[k][live]) <= GEN_GATE, (f, k)
        assert scaled(got["canvas"][f], want["canvas"]) <= GEN_GATE, f
    assert present > 0


def _two_cores(flags, hw, options=None):
    F = make_flags(**flags)
    P = params32(F, hw, 3, 0.05)
    cores = []
    for _ in range(2):
        c = SqairCore(F, hw, options=options)
        c.set_params(P)
        cores.append(c)
    return F, cores


@pytest.mark.parametrize("smc", [False, True])
@pytest.mark.parametrize("chain", [False, True])
def test_forecasting_between_steps_changes_nothing(smc, chain):
    hw, B, steps = (50, 50), 4, 6
    F, (ca, cb) = _two_cores(dict(k_particles=4, n_steps_per_image=3), hw, options={"slot_chain": 1} if chain else None)
    obs = _frames(hw, B, steps, 31)
    kw = dict(resample="systematic", ess_frac=0.7) if smc else {}
    sa, sb = SqairStream(ca, B, seed=5, **kw), SqairStream(cb, B, seed=5, **kw)
    for s in range(steps):
        if s == 3:   # a reset armed before a forecast
            sa.reset([1])
            sb.reset([1])
        fc = sa.forecast(3 + s % 2)
        oa, ob = host(sa.step(obs[s:s + 1])), host(sb.step(obs[s:s + 1]))
        torch.cuda.synchronize()
        if chain:
            ca.check_chain()
            cb.check_chain()
        assert np.isfinite(fc["canvas"].cpu().numpy()).all()
        for k in ob:
            assert np.array_equal(oa[k], ob[k], equal_nan=True), (s, k)
        assert torch.equal(sa.state.view(torch.int32), sb.state.view(torch.int32)), s   # (the blob's bytes)
        assert torch.equal(sa.log_weight_sum, sb.log_weight_sum), s
        if smc:
            for k in ("log_z", "ess", "_src", "resampled", "log_evidence"):
                assert torch.equal(getattr(sa, k), getattr(sb, k)), (s, k)
        assert (sa._armed is None) == (sb._armed is None) and sa._src_is_identity == sb._src_is_identity
    assert len(sa._fc) == 1   # (two horizons were asked for: only the last one's buffers are kept)


def _raw(st, Fn, noise, src, log_w=None, summaries=True, capture=False):
    """sqair_forecast on caller buffers (the stream's handle and state): {name: device tensor}."""
    core = st.core
    R, B, N = st.R, st.B, core.N
    z = lambda *shp: torch.zeros(shp, dtype=torch.float32, device=core.device)
    out = dict(what=z(Fn, R, N, core.nw), where=z(Fn, R, N, 4), presence=z(Fn, R, N), obj_id=z(Fn, R, N), canvas=z(Fn, R, core.H, core.W))
    if summaries:
        out.update(mean_canvas=z(Fn, B, core.H, core.W), expected_count=z(Fn, B))
    c_out = _capi.SqairForecastOutputs(**{k: v.data_ptr() for k, v in out.items()})
    c_out.log_w = None if log_w is None else log_w.data_ptr()
    ws = z(core.lib.sqair_forecast_workspace_bytes(core.handle, Fn, B) // 4)
    nz = torch.as_tensor(noise, dtype=torch.float32, device=core.device).contiguous()
    s = torch.cuda.Stream(device=core.device)
    s.wait_stream(torch.cuda.current_stream())
    ss = C.c_void_p(s.cuda_stream)
    args = (core.handle, core.flat.data_ptr(), core.packed.data_ptr(), nz.data_ptr(), Fn, B, None if src is None else src.data_ptr(),
            C.byref(c_out), ws.data_ptr(), ws.numel() * 4, ss)
    if capture:
        core.check(core.lib.sqair_capture_begin(core.handle, ss), "sqair_capture_begin")
        core.check(core.lib.sqair_forecast(*args), "sqair_forecast")
        nodes = core.lib.sqair_capture_end(core.handle, ss, 3)
        assert nodes > 0, nodes
        for v in out.values():
            v.fill_(-7.0)
        torch.cuda.synchronize()
        core.check(core.lib.sqair_capture_launch(core.handle, 3, ss), "sqair_capture_launch")
    else:
        core.check(core.lib.sqair_forecast(*args), "sqair_forecast")
    s.synchronize()
    return out


def test_pending_map_reset_and_resampled_rows():
    hw, B, Fn = (32, 40), 3, 4
    flags = dict(k_particles=4, n_steps_per_image=3)
    F, P, obs, core = _setup(flags, hw, B, 3)
    K, N, nzw = 4, 3, 4 + int(F.n_what) + 1
    R = B * K
    rng = np.random.default_rng(9)
    # reset: lane j's rows forecast from the initial state
    noise = draw_noise(rng, 2, R, N, nzw)
    st = SqairStream(core, B, frames_per_step=2, use_graph=False)
    st.step(obs[:2], noise=noise)
    st.reset([1])
    orc = O.SqairOracle(P, O.make_cfg(F, hw), torch.float64)
    rows = slice(K, 2 * K)
    for attempt in range(DRAWS):   # (decision-stable on the oracle's margins alone)
        fnoise = draw_noise(rng, Fn, R, N, nzw)
        ref = forecast_ref(orc, orc.initial_state(R), fnoise)
        if float(prior_margin(ref, fnoise)[rows].min()) >= MARGIN:
            break
    got = host(st.forecast(Fn, noise=fnoise))
    assert np.array_equal(got["presence"][:, rows], ref["presence"][:, rows].numpy().astype(np.float32))
    assert np.array_equal(got["obj_id"][:, rows], ref["obj_id"][:, rows].numpy().astype(np.float32))
    for k in ("what", "where", "canvas"):
        assert scaled(got[k][:, rows], ref[k][:, rows].numpy()) <= GATE, k
    assert np.array_equal(got["weights"][1], np.full(K, 1.0 / K, np.float32))   # (a reset lane's weights start at zero)
    st.close()
    # SMC that resampled: row r of the forecast is the forecast of its ancestor row (one noise row for every row)
    core2 = SqairCore(F, hw)
    core2.set_params(P)
    sm = SqairStream(core2, B, frames_per_step=1, resample="systematic", ess_frac=1.0, seed=3, use_graph=False)
    for s in range(2):
        sm.step(obs[s:s + 1])
    torch.cuda.synchronize()
    assert sm.resampled.cpu().numpy().all()
    anc = sm._src.cpu().numpy()
    one = np.broadcast_to(draw_noise(rng, Fn, 1, N, nzw), (Fn, R, 2, N, nzw)).copy()
    got = host(sm.forecast(Fn, noise=one, summaries=False))
    ident = torch.arange(R, dtype=torch.int32, device=core2.device)
    base = host(_raw(sm, Fn, one, ident, summaries=False))
    assert not np.array_equal(anc, np.arange(R))
    for k in ("what", "where", "presence", "obj_id", "canvas"):
        assert np.array_equal(got[k], base[k][:, anc]), k


def test_summaries():
    hw, B, Fn = (32, 40), 3, 3
    F, P, obs, core = _setup(dict(k_particles=4, n_steps_per_image=3), hw, B, 2)
    K, N, nzw = 4, 3, 4 + int(F.n_what) + 1
    R = B * K
    st = SqairStream(core, B, frames_per_step=2, use_graph=False)
    st.step(obs)
    noise = draw_noise(np.random.default_rng(4), Fn, R, N, nzw)
    dev = core.device
    ident = torch.arange(R, dtype=torch.int32, device=dev)
    lw = torch.as_tensor(np.random.default_rng(1).normal(0, 3, R).astype(np.float32), device=dev)
    a = host(_raw(st, Fn, noise, ident, lw))
    w = np.exp(lw.cpu().numpy().astype(np.float64).reshape(B, K))
    w /= w.sum(1, keepdims=True)
    cv = a["canvas"].astype(np.float64).reshape(Fn, B, K, -1)
    cnt = a["presence"].astype(np.float64).reshape(Fn, B, K, N).sum(-1)
    want_mc = np.einsum("bk,fbkp->fbp", w, cv).reshape(a["mean_canvas"].shape)
    want_ec = np.einsum("bk,fbk->fb", w, cnt)
    assert np.abs(a["mean_canvas"] - want_mc).max() <= 1e-5 * np.abs(want_mc).max()
    assert np.abs(a["expected_count"] - want_ec).max() <= 1e-5 * max(1.0, np.abs(want_ec).max())
    b = host(_raw(st, Fn, noise, ident, lw))
    for k in a:
        assert np.array_equal(a[k], b[k]), k   # two calls, the same bits
    # uniform when log_w is NULL
    u = host(_raw(st, Fn, noise, ident, None))
    assert np.abs(u["mean_canvas"] - cv.mean(2).reshape(u["mean_canvas"].shape)).max() <= 1e-5 * np.abs(cv).max()
    assert np.abs(u["expected_count"] - cnt.mean(2)).max() <= 1e-5 * max(1.0, cnt.max())
    # one finite weight: exactly that particle's canvas; a NaN, or every weight at -inf: NaN
    lw2 = torch.full((R,), -float("inf"), device=dev)
    lw2[0 * K + 2] = 1.5                        # lane 0: particle 2 alone
    lw2[1 * K + 1] = float("nan")               # lane 1: a NaN among -inf
    e = host(_raw(st, Fn, noise, ident, lw2))   # lane 2: all -inf
    mc = e["mean_canvas"].reshape(Fn, B, -1)
    assert np.array_equal(mc[:, 0], e["canvas"].reshape(Fn, B, K, -1)[:, 0, 2])
    assert np.array_equal(e["expected_count"][:, 0], cnt[:, 0, 2].astype(np.float32))
    assert np.isnan(mc[:, 1:]).all() and np.isnan(e["expected_count"][:, 1:]).all()
    # a lane with a +inf weight: NaN too
    lw3 = lw.clone()
    lw3[K] = float("inf")
    g = host(_raw(st, Fn, noise, ident, lw3))
    assert np.isnan(g["expected_count"][:, 1]).all() and np.isfinite(g["expected_count"][:, [0, 2]]).all()
    st.close()


def test_captured_forecast_replays_the_eager_call():
    hw, B, Fn = (50, 50), 4, 5
    F, P, obs, core = _setup(dict(k_particles=5, n_steps_per_image=3), hw, B, 2)
    K, N, nzw = 5, 3, 4 + int(F.n_what) + 1
    st = SqairStream(core, B, frames_per_step=2, resample="systematic", ess_frac=0.5)
    st.step(obs)
    torch.cuda.synchronize()
    noise = draw_noise(np.random.default_rng(2), Fn, B * K, N, nzw)
    eager = host(_raw(st, Fn, noise, st._src, st.log_weight_sum))
    graph = host(_raw(st, Fn, noise, st._src, st.log_weight_sum, capture=True))
    for k in eager:
        assert np.array_equal(eager[k], graph[k]), k
    assert eager["presence"].sum() > 0
