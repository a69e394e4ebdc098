"""-m gpu: missing-frame steps (include/sqair_hip.h: sqair_set_observed; SqairStream(missing=True).step(observed=...)).

A mixed mask against the fp64 reference of tests/coast_ref.py -- every bound output, the zeros included --; a run of steps without
any frame against forecast(); the frames of unobserved lanes not mattering; a mask with every lane observed against a stream
without one; SMC left alone by a coasted step and a gappy stream as a particle filter against the oracle; one captured graph
for every mask and its node count; a pass of several frames against one-frame steps; the slot chain; the track history.

Noise is picked on the REFERENCE's margins alone (the first of DRAWS draws whose posterior and prior presence decisions are at
least MARGIN from flipping), and what a case is meant to reach is asserted on the reference before the HIP path runs.  Gates:
presence and obj_id exactly, the rest within 5e-4 scaled error (tests/test_forecast.py), HIP against HIP bit for bit."""
import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from sqair_amd.model import SqairCore
from sqair_amd.stream import FORECAST_OUTPUTS, SqairStream
from tests import history_ref as H
from tests import smc_ref as S
from tests.coast_ref import COASTED, COUNTS, coast_ref
from tests.hip_util import MARGIN, draw_noise
from tests.stream_harness import core as make_core, host, scaled as _scaled, setup

pytestmark = pytest.mark.gpu

GATE = 5e-4        # live-oracle gate (scaled absolute error), tests/test_forecast.py
REL = 1e-4         # log weights and evidence of the particle filter (tests/test_smc_oracle.py)
DRAWS = 6
EXACT = ("presence", "obj_id")
ALL = tuple(_capi.OUTPUT_FIELDS[:_capi.N_REFERENCE_OUTPUTS])
HW = (32, 40)
LSTM = dict(time_transition="LSTM", prior_transition="LSTM")
T = 6

# name: (flags, B).  prop_prior_step_bias = 1: a prior presence probability near 0.7, so that coasted frames drop objects (the
# default, 10, keeps every coasted object alive)
CASES = {
    "gru": (dict(k_particles=3, n_steps_per_image=3), 3),
    "gru_drops": (dict(k_particles=3, n_steps_per_image=3, prop_prior_step_bias=1.0), 3),
    "lstm": (dict(k_particles=3, n_steps_per_image=2, **LSTM), 2),
    "rw": (dict(k_particles=3, n_steps_per_image=3, prop_prior_type="rw"), 2),
    "guided": (dict(k_particles=3, n_steps_per_image=3, prop_prior_type="guided", rec_where_prior=True), 2),
    "padded_n_units": (dict(k_particles=2, n_steps_per_image=3, n_units=5), 2),
    "wide_n_what_64": (dict(k_particles=2, n_steps_per_image=3, n_what=64), 2),
    "k1": (dict(k_particles=1, n_steps_per_image=3), 4),
}


def pattern(frames, B):
    """observed [frames, B]: lane b sees frame 0, then has a gap of two frames starting at 1 + b (mod frames - 1) -- observed, two
    unobserved, observed again for every lane whose gap ends before the clip does."""
    m = np.ones((frames, B), bool)
    for b in range(B):
        g = 1 + b % (frames - 1)
        m[g:g + 2, b] = False
    return m


def _setup(flags, B, frames=T, seed=19, hw=HW, options=None, cores=1):
    F, P, obs, _ = setup(flags, B, frames, hw, seed)
    return F, P, obs, [make_core(F, hw, P, options) for _ in range(cores)]


def _dims(F, B):
    K, N = int(F.k_particles), int(F.n_steps_per_image)
    return K, N, 4 + int(F.n_what) + 1, B * K


def gap_starts(mask):
    """(t, b) of every unobserved (frame, lane) whose lane was observed at t - 1."""
    return [(t, b) for t in range(1, mask.shape[0]) for b in range(mask.shape[1]) if not mask[t, b] and mask[t - 1, b]]


def reference(F, P, obs, B, mask, hw=HW):
    """CPU: coast_ref over the clip on the first decision-stable noise draw.  Returns (noise, reference outputs, margin)."""
    K, N, nzw, R = _dims(F, B)
    orc = O.SqairOracle(P, O.make_cfg(F, hw), torch.float64)
    tiled = O.tile_input_for_iwae(torch.as_tensor(obs, dtype=torch.float64), K)
    rng = np.random.default_rng(23)
    for attempt in range(DRAWS):
        noise = draw_noise(rng, mask.shape[0], R, N, nzw)
        ref, _ = coast_ref(orc, orc.initial_state(R), tiled, noise, mask)
        mg = min(float(ref["presence_margins"].min()), float(ref["prior_margin"].min()))
        if mg >= MARGIN:
            return noise, ref, mg
    raise AssertionError("no decision-stable noise draw in {} attempts (last margin {:.2e})".format(DRAWS, mg))


def reach(ref, mask, K):
    """What the reference rollout reaches: objects present in a lane when its gap begins, and coasted frames that drop an object
    which is not the last present one of its row."""
    pres = ref["presence"].numpy()
    alive = sum(int(pres[t - 1, b * K:(b + 1) * K].sum()) for t, b in gap_starts(mask))
    drops = 0
    for t in range(1, mask.shape[0]):
        for b in np.flatnonzero(~mask[t]):
            for r in range(b * K, (b + 1) * K):
                before, after = pres[t - 1, r], pres[t, r]
                ids_b, ids_a = ref["obj_id"].numpy()[t - 1, r], ref["obj_id"].numpy()[t, r]
                live = [i for i, p in zip(ids_b, before) if p > 0]
                kept = [i for i, p in zip(ids_a, after) if p > 0]
                drops += int(any(i not in kept for i in live[:-1]) and len(kept) > 0)
    return alive, drops


# ---- 1. a mixed mask against the fp64 reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_mixed_mask_matches_the_fp64_reference(case):
    flags, B = CASES[case]
    F, P, obs, (core,) = _setup(flags, B)
    K, N, nzw, R = _dims(F, B)
    if "n_what" in flags:
        assert core.lib is _capi.lib(_capi.WIDE_LIB_PATH)
    mask = pattern(T, B)
    assert any(mask[t - 1, b] and not mask[t, b] and not mask[t + 1, b] and mask[t + 2, b] for t in range(1, T - 2) for b in range(B))
    noise, ref, mg = reference(F, P, obs, B, mask)
    alive, drops = reach(ref, mask, K)
    assert alive > 0, "no object is present in an unobserved lane when its gap begins"
    if case == "gru_drops":
        assert drops > 0, "no coasted frame drops an object that is not the last one"
    st = SqairStream(core, B, outputs=ALL, use_graph=False, missing=True)
    worst = {}
    for t in range(T):
        frames = obs[t:t + 1].copy()
        got = host(st.step(frames, noise=noise[t:t + 1], observed=mask[t]))
        assert np.array_equal(got.pop("observed"), mask[t:t + 1])
        rows = np.repeat(mask[t], K)
        for k in ALL:
            want = ref[k][t].numpy()
            g = got[k][0].reshape(want.shape)
            if k in EXACT:
                assert np.array_equal(g, want.astype(np.float32)), (t, k)
                continue
            e = _scaled(g, want)
            worst[k] = max(worst.get(k, 0.0), e)
            assert e <= GATE, (t, k, e)
            if k not in COASTED and k not in COUNTS:   # written as 0, not as something small
                assert not g[~rows].any(), (t, k)
            elif k in COUNTS:
                assert np.array_equal(g[~rows], want[~rows].astype(np.float32)), (t, k)
    print(case, "margin {:.4f}".format(mg), "alive at gap starts", alive, "mid drops", drops,
          {k: "{:.1e}".format(v) for k, v in worst.items() if v > 1e-5})
    st.close()


# ---- 2. no lane observed for F steps is forecast(F) ------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_steps_without_any_frame_are_the_forecast(cell):
    flags = dict(k_particles=3, n_steps_per_image=3, prop_prior_step_bias=2.0, **(LSTM if cell == "lstm" else {}))
    B, S_, Fn = 2, 3, 4
    F, P, obs, (ca, cb) = _setup(flags, B, frames=S_, cores=2)
    K, N, nzw, R = _dims(F, B)
    rng = np.random.default_rng(3)
    noise, fnoise = draw_noise(rng, S_, R, N, nzw), draw_noise(rng, Fn + 2, R, N, nzw)
    sa = SqairStream(ca, B, outputs=ALL, use_graph=False, missing=True)
    sb = SqairStream(cb, B, use_graph=False)
    for t in range(S_):
        sa.step(obs[t:t + 1], noise=noise[t:t + 1])
        sb.step(obs[t:t + 1], noise=noise[t:t + 1])
    want = host(sb.forecast(Fn + 2, noise=fnoise))
    assert want["presence"][:Fn].sum() > 0 and want["presence"][Fn - 1].sum() < want["presence"][0].sum()   # objects, and some die
    none = np.zeros(B, bool)
    blank = np.zeros((1, B) + HW, np.float32)
    for f in range(Fn):
        got = host(sa.step(blank, noise=fnoise[f:f + 1], observed=none))
        for k in FORECAST_OUTPUTS:
            assert np.array_equal(got[k][0], want[k][f]), (f, k)
        assert not got["log_weights_per_timestep"].any()
    # the state after the F steps: a further forecast from it continues the long one
    more = host(sa.forecast(2, noise=fnoise[Fn:]))
    for k in FORECAST_OUTPUTS + ("mean_canvas", "expected_count", "weights"):
        assert np.array_equal(more[k], want[k][Fn:] if k != "weights" else want[k]), k
    sa.close()
    sb.close()


# ---- 3. the frames of unobserved lanes do not matter -----------------------------------------------------------------------------
def _stream_state(st):
    d = dict(state=st.state.view(torch.int32), log_weight_sum=st.log_weight_sum)
    if st.smc:
        d.update({k: getattr(st, k) for k in ("log_z", "ess", "_src", "resampled", "log_evidence")})
    return {k: v.clone() for k, v in d.items()}


def _same_streams(a, b, tag):
    for k, v in _stream_state(a).items():
        assert torch.equal(v, _stream_state(b)[k]), (tag, k)


def test_frames_of_unobserved_lanes_do_not_matter():
    B = 3
    F, P, obs, cores = _setup(dict(k_particles=3, n_steps_per_image=3), B, cores=3)
    K, N, nzw, R = _dims(F, B)
    mask = pattern(T, B)
    noise = draw_noise(np.random.default_rng(8), T, R, N, nzw)
    kw = dict(outputs=ALL, resample="systematic", ess_frac=0.5, seed=2, missing=True)
    s1, s2, s3 = (SqairStream(c, B, **kw) for c in cores)
    # the C ABI takes the frames as they are: two streams whose unobserved lanes hold different finite frames
    s1._blank_unobserved = s2._blank_unobserved = lambda frames, observed: frames
    rng = np.random.default_rng(1)
    for t in range(T):
        gone = torch.as_tensor(~mask[t])
        f1, f2, f3 = (torch.as_tensor(obs[t:t + 1].copy()) for _ in range(3))
        f1[0, gone] = torch.as_tensor(rng.uniform(size=(int(gone.sum()),) + HW).astype(np.float32))
        f2[0, gone] = 1.0 - f1[0, gone] * 0.5
        f3[0, gone] = float("nan")     # through Python anything goes: the stream blanks the lane
        u = rng.uniform(size=B).astype(np.float32)
        o1, o2, o3 = (host(s.step(f, noise=noise[t:t + 1], uniforms=u, observed=mask[t])) for s, f in ((s1, f1), (s2, f2), (s3, f3)))
        for k in o1:
            assert np.array_equal(o1[k], o2[k], equal_nan=True) and np.array_equal(o1[k], o3[k], equal_nan=True), (t, k)
            assert np.isfinite(o1[k]).all(), (t, k)
        _same_streams(s1, s2, t)
        _same_streams(s1, s3, t)
    for s in (s1, s2, s3):
        s.close()


# ---- 4. a mask with every lane observed is no mask -------------------------------------------------------------------------------
def test_every_lane_observed_equals_a_stream_without_a_mask():
    B = 3
    F, P, obs, (ca, cb) = _setup(dict(k_particles=3, n_steps_per_image=3), B, cores=2)
    kw = dict(outputs=ALL, resample="systematic", ess_frac=0.5, seed=9)
    sa, sb = SqairStream(ca, B, missing=True, **kw), SqairStream(cb, B, **kw)
    for t in range(T):
        oa = host(sa.step(obs[t:t + 1], observed=None if t % 2 else np.ones(B, bool)))
        ob = host(sb.step(obs[t:t + 1]))
        assert oa.pop("observed").all() and "observed" not in ob
        for k in ob:
            assert np.array_equal(oa[k], ob[k], equal_nan=True), (t, k)
        _same_streams(sa, sb, t)
    with pytest.raises(ValueError, match="missing=True"):
        sb.step(obs[:1], observed=np.ones(B, bool))
    sa.close()
    sb.close()


# ---- 5. SMC ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frac", [0.5, 1.0])
def test_a_coasted_step_leaves_the_lanes_weights_alone(frac):
    """log_evidence and the carried log weights of an unobserved lane are exactly what they were.  So is its ESS, the ESS of the
    weights the lane carries: after a step in which the lane resampled these are uniform, ESS = K exactly (the ess output of that
    step was taken before its resampling), and the resampler -- which at ess_frac = 1 runs on the coasted step too -- then writes
    the identity map."""
    B, K, frames = 3, 4, 8
    F, P, obs, (core,) = _setup(dict(k_particles=K, n_steps_per_image=2), B, frames=frames)
    st = SqairStream(core, B, resample="systematic", ess_frac=frac, seed=41, missing=True)
    mask = pattern(frames, B)
    mask[5] = False      # a step nobody sees
    seen = dict(coasted=0, after_resampling=0, carried=0)
    prev = None
    for t in range(frames):
        lw0 = st.log_weight_sum.clone()
        o = host(st.step(obs[t:t + 1], observed=mask[t]))
        lw1 = st.log_weight_sum.cpu().numpy()
        for b in np.flatnonzero(~mask[t]):
            rows = slice(b * K, (b + 1) * K)
            assert not o["log_weights_per_timestep"][0, rows].any()
            if prev is None:
                continue
            seen["coasted"] += 1
            assert o["log_evidence"][b] == prev["log_evidence"][b], (t, b)
            assert np.array_equal(lw1[rows], lw0.cpu().numpy()[rows]), (t, b)
            assert np.array_equal(o["ancestors"][rows], np.arange(b * K, (b + 1) * K)), (t, b)
            if prev["resampled"][b]:
                seen["after_resampling"] += 1
                assert o["ess"][b] == K and not lw1[rows].any(), (t, b)
            else:
                seen["carried"] += 1
                assert o["ess"][b] == prev["ess"][b] and o["resampled"][b] == 0, (t, b)
        prev = o
    print(frac, seen)
    assert seen["coasted"] >= 6 and seen["after_resampling"] > 0
    assert seen["carried"] > 0 or frac == 1.0
    st.close()


def test_gappy_stream_matches_the_fp64_particle_filter():
    flags, B, frames, frac = dict(k_particles=4, n_steps_per_image=2), 3, 10, 0.5
    F, P, obs, (core,) = _setup(flags, B, frames=frames)
    K, N, nzw, R = _dims(F, B)
    outs = ("what", "where", "presence", "obj_id", "presence_prob", "log_weights_per_timestep")
    st = SqairStream(core, B, outputs=outs, seed=41, resample="systematic", ess_frac=frac, missing=True)
    pf = S.ParticleFilter(P, F, HW, B)
    mask = pattern(frames, B)
    mask[6:8, 0] = False     # a second gap
    rng = np.random.default_rng(7)
    went = coasted_alive = 0
    for s in range(frames):
        tiled = O.tile_input_for_iwae(torch.as_tensor(obs[s:s + 1], dtype=torch.float64), K)
        for attempt in range(DRAWS):   # the oracle's own margins decide; the device is not looked at
            noise = draw_noise(rng, 1, R, N, nzw)
            prop = coast_ref(pf.orc, pf.state, tiled, noise, mask[s:s + 1])
            if min(float(prop[0]["presence_margins"].min()), float(prop[0]["prior_margin"].min())) >= MARGIN:
                break
        else:
            raise AssertionError("no decision-stable noise draw in {} attempts at step {}".format(DRAWS, s))
        lw0_ref, lz0_ref = pf.log_w.copy(), pf.log_z.copy()
        ref, rw = pf.commit(prop)
        lw0 = st.log_weight_sum.cpu().numpy()
        o = host(st.step(obs[s:s + 1], noise=noise, observed=mask[s]))
        # the Philox uniform is keyed by the lane's frame counter after the step: a coasted frame is time that passed
        assert np.array_equal(st.u.cpu().numpy(), S.smc_uniform(np.arange(B), pf.state.t.numpy()[::K], 41)), s
        for k in EXACT:
            want = ref[k].numpy()
            assert np.array_equal(o[k].reshape(want.shape), want.astype(np.float32)), (s, k)
        for k in ("what", "where", "presence_prob"):
            assert _scaled(o[k], ref[k].numpy()) <= GATE, (s, k)
        coasted_alive += int(ref["presence"].numpy()[0][np.repeat(~mask[s], K)].sum())
        lw_ref = ref["log_weights_per_timestep"].numpy()
        assert float((np.abs(o["log_weights_per_timestep"] - lw_ref) / np.maximum(1.0, np.abs(lw_ref))).max()) <= REL, s
        a_dev = S.accumulate(lw0, o["log_weights_per_timestep"]).astype(np.float64)
        a_scale = np.maximum.reduce([np.ones(R), np.abs(pf.a), np.abs(lw0_ref), np.abs(lw_ref).max(0)])
        assert float((np.abs(a_dev - pf.a) / a_scale).max()) <= REL, (s, "a_k")
        ev_scale = np.maximum.reduce([np.ones(B), np.abs(rw.log_evidence), np.abs(lz0_ref), np.abs(rw.w.m)])
        assert float((np.abs(o["log_evidence"] - rw.log_evidence) / ev_scale).max()) <= REL, (s, "log_evidence")
        delta = np.abs(a_dev - pf.a).reshape(B, K).max(1)
        for b in range(B):   # decisions on the oracle's ESS, skipped only where the measured log-weight discrepancy allows a flip
            if abs(rw.ess[b] - frac * K) > (8 * delta[b] + 1e-5) * rw.ess[b]:
                assert bool(o["resampled"][b]) == bool(rw.ess[b] < frac * K), (s, b)
            if not mask[s, b]:
                assert not o["resampled"][b], (s, b)   # (a coasted lane carried weights that did not ask for resampling before)
        went += int(o["resampled"].sum())
        pf.advance(o["ancestors"].astype(np.int64), o["resampled"].astype(bool))   # the filter follows the device's map
    assert went > 0 and coasted_alive > 0, (went, coasted_alive)
    st.close()


# ---- 6. one graph for every mask ------------------------------------------------------------------------------------------------
def _count_captures(core):
    seen, check = [], core.check

    def counting(rc, what):
        seen.append(what)
        return check(rc, what)
    core.check = counting
    return lambda: seen.count("sqair_graph_capture")


def test_one_graph_serves_every_mask():
    B, frames = 3, 8
    F, P, obs, (ca, cb) = _setup(dict(k_particles=3, n_steps_per_image=3), B, frames=frames, cores=2)
    mask = pattern(frames, B)
    mask[4] = True       # a step with every lane observed
    mask[6] = False      # ... and one with none
    assert len({tuple(m) for m in mask}) >= 5
    kw = dict(outputs=ALL, resample="systematic", ess_frac=0.5, seed=4, missing=True, history=4)
    sg, se = SqairStream(ca, B, use_graph=True, **kw), SqairStream(cb, B, use_graph=False, **kw)
    captures = _count_captures(ca)
    for t in range(frames):
        og, oe = host(sg.step(obs[t:t + 1], observed=mask[t])), host(se.step(obs[t:t + 1], observed=mask[t]))
        for k in oe:
            assert np.array_equal(og[k], oe[k], equal_nan=True), (t, k)
        _same_streams(sg, se, t)
    assert captures() == 1
    tg, te = host(sg.tracks()), host(se.tracks())
    for k in te:
        assert H.same_bits(tg[k], te[k]), k
    sg.close()
    se.close()


@pytest.mark.parametrize("TS", [1, 4])
def test_graph_has_exactly_frames_plus_one_nodes_more(TS):
    B = 2
    F, P, obs, _ = _setup(dict(k_particles=2, n_steps_per_image=3), B, frames=TS, cores=0)

    def nodes(**kw):
        core = SqairCore(F, HW)
        core.set_params(P)
        st = SqairStream(core, B, frames_per_step=TS, **kw)
        st.step(obs)
        torch.cuda.synchronize()
        return core.graph_nodes()

    plain = nodes()
    assert plain > 50 and nodes(missing=False) == plain
    assert nodes(missing=True) == plain + TS + 1
    assert nodes(missing=True, resample="systematic", history=3) == plain + TS + 3


# ---- 7. a pass of four frames with a per-frame mask is four one-frame steps --------------------------------------------------------
def test_a_pass_of_four_frames_equals_four_steps():
    B, TS = 3, 4
    F, P, obs, (ca, cb) = _setup(dict(k_particles=3, n_steps_per_image=3), B, frames=2 * TS, cores=2)
    K, N, nzw, R = _dims(F, B)
    mask = pattern(2 * TS, B)
    mask[5] = False
    noise = draw_noise(np.random.default_rng(6), 2 * TS, R, N, nzw)
    # (ess_frac = 0: the resampler never resamples, it only accumulates the log weights on the device, in frame order -- the
    #  same fp32 sums whether the frames come one by one or four at a time)
    kw = dict(outputs=ALL, missing=True, resample="systematic", ess_frac=0.0)
    s4, s1 = SqairStream(ca, B, frames_per_step=TS, **kw), SqairStream(cb, B, frames_per_step=1, **kw)
    present = 0
    for c in range(2):
        fr = slice(c * TS, (c + 1) * TS)
        o4 = host(s4.step(obs[fr], noise=noise[fr], observed=mask[fr]))
        for i, t in enumerate(range(fr.start, fr.stop)):
            o1 = host(s1.step(obs[t:t + 1], noise=noise[t:t + 1], observed=mask[t]))
            for k in ALL + ("observed",):
                assert np.array_equal(o4[k][i], o1[k][0], equal_nan=True), (t, k)
            present += int(o1["presence"][0][np.repeat(~mask[t], K)].sum())
        _same_streams(s4, s1, c)
    assert present > 0
    with pytest.raises(ValueError, match=r"\[4, 3\] expected"):
        s4.step(obs[:TS], observed=np.ones(B, bool))
    s4.close()
    s1.close()


# ---- 8. the slot chain -----------------------------------------------------------------------------------------------------------
def test_slot_chain_equals_the_launches():
    B, hw = 4, (50, 50)
    flags = dict(k_particles=4, n_steps_per_image=3)
    F, P, obs, (ca,) = _setup(flags, B, hw=hw, seed=31, options={"slot_chain": 1})
    cb = SqairCore(F, hw)
    cb.set_params(P)
    mask = pattern(T, B)
    kw = dict(outputs=ALL, resample="systematic", ess_frac=0.7, seed=5, missing=True)
    sa, sb = SqairStream(ca, B, **kw), SqairStream(cb, B, **kw)
    present = 0
    for t in range(T):
        oa, ob = host(sa.step(obs[t:t + 1], observed=mask[t])), host(sb.step(obs[t:t + 1], observed=mask[t]))
        ca.check_chain()
        for k in ob:
            assert np.array_equal(oa[k], ob[k], equal_nan=True), (t, k)
        _same_streams(sa, sb, t)
        present += int(ob["presence"][0][np.repeat(~mask[t], 4)].sum())
    assert present > 0
    sa.close()
    sb.close()


# ---- 9. the track history records the coasted frames -----------------------------------------------------------------------------
def test_tracks_return_the_coasted_frames():
    B, K, L, frames = 3, 3, 8, 7
    F, P, obs, (core,) = _setup(dict(k_particles=K, n_steps_per_image=3), B, frames=frames)
    st = SqairStream(core, B, outputs=("what", "where", "presence", "obj_id", "log_weights_per_timestep"), history=L, missing=True)
    mask = pattern(frames, B)
    fields = dict(where="where", presence="presence", obj_id="obj_id", what="what", log_w="log_weights_per_timestep")
    rec, steps = H.Recorder(B * K), []
    for t in range(frames):
        parent = st.carried.pending().copy()
        o = host(st.step(obs[t:t + 1], observed=mask[t]))
        rec.push(parent, **{k: o[v] for k, v in fields.items()})
        steps.append(o)
    got = host(st.tracks(start="last"))
    want = H.trace(rec.steps, L, L, K, None, 2 * core.N)
    for k, v in want.items():
        assert got[k].dtype == v.dtype and H.same_bits(got[k], v), k
    # frame f of the trace is step f (7 steps in a ring of 8: the oldest frame is invalid): the gap frames hold the coasted outputs
    off, alive = L - frames, 0
    for t in range(frames):
        gone = np.repeat(~mask[t], K)
        for k in ("where", "presence", "obj_id"):
            assert np.array_equal(got[k][off + t][gone], steps[t][k][0][gone]), (t, k)
        assert not got["log_w"][off + t][gone].any()
        alive += int(got["presence"][off + t][gone].sum())
    assert alive > 0
    st.close()
