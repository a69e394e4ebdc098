"""The stream-level cases more than one file runs: a forecast against the fp64 rollout (tests/test_forecast.py), a resampling stream
against the fp64 particle filter (tests/test_smc_oracle.py) and chunk two of a trained stream against the oracle started from its own
state (tests/test_stream_train.py).  tests/test_presence_paths.py, test_regime_paths.py and test_latent_regimes.py run them again on
other parameters through `edits` and `require`.  What these cases expect -- the gates, the draws, what is exact -- is stated here, in
the shape of tests/pass_cases.py; how they obtain what they judge is tests/stream_harness.py.  Importable without a GPU.

Not rewritten by pytest, so every assert here carries what it compared."""
import numpy as np
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from sqair_amd.train import StreamTrainer
from tests import smc_ref as S
from tests import tbptt_ref
from tests.forecast_ref import forecast_ref, prior_margin
from tests.hip_util import MARGIN, presence_margins
from tests.pass_cases import check_report
from tests.stream_harness import differ, accumulate, core, frames, host, noise, scaled, setup, train_setup

ORACLE_HW = (32, 40)
ORACLE_GATE = 5e-4   # live-oracle gate (scaled absolute error) of the per-frame outputs
ORACLE_REL = 1e-4    # north-star bar: log weights and evidence (relative to max(1, the value, the terms summed into it))
DRAWS = 6            # noise draws before giving up on a decision-stable one
EXACT = ("presence", "obj_id")
CLOSE = ("what", "where", "presence_prob", "presence_logit", "canvas", "glimpse")
FILTER_OUTS = ("what", "where", "presence", "obj_id", "presence_prob", "log_weights_per_timestep")


def reference_rollout(F, P, obs, hw, B, S_, Fn):
    """CPU: the oracle over the S_ streamed frames and the fp64 rollout of Fn frames from its state, on the first of DRAWS noise
    draws whose ORACLE margins (the posterior presences and the forecast's prior draws) are decision-stable.  Returns
    (noise, forecast noise, reference rollout, the state it started from, margin)."""
    K = int(F.k_particles)
    R = B * K
    orc = O.SqairOracle(P, O.make_cfg(F, hw), torch.float64)
    tiled = O.tile_input_for_iwae(torch.as_tensor(obs, dtype=torch.float64), K)
    rng = np.random.default_rng(23)
    for attempt in range(DRAWS):   # the oracle's margins alone decide: the posterior presences and the forecast's prior draws
        nz, fnoise = noise(F, rng, S_, R), noise(F, rng, Fn, R)
        with torch.no_grad():
            seq, state = orc.sequence(tiled, torch.as_tensor(nz, dtype=torch.float64), state=orc.initial_state(R), return_state=True)
        ref = forecast_ref(orc, state, fnoise)
        mg = min(float(presence_margins(seq, nz).min()), float(prior_margin(ref, fnoise).min()))
        if mg >= MARGIN:
            return nz, fnoise, ref, state, mg
    raise AssertionError("no decision-stable noise draw in {} attempts (last margin {:.2e})".format(DRAWS, mg))


def rollout_case(case, flags, hw, B, S_, Fn, require=None, edits=None):
    """A stream over S_ frames (data seed 19), then a forecast of Fn frames against the fp64 rollout.  require(ref, state): a condition
    on the REFERENCE rollout alone (what the case is meant to reach), checked before the HIP path runs."""
    F, P, obs, _ = setup(flags, B, S_, hw, 19, edits=edits, obs=frames(hw, B, S_, 19))
    c = core(F, hw, P)
    K = int(F.k_particles)
    if "n_what" in flags:
        assert c.lib is _capi.lib(_capi.WIDE_LIB_PATH), "the wide library was meant to serve this case"
    nz, fnoise, ref, state, mg = reference_rollout(F, P, obs, hw, B, S_, Fn)
    if require is not None:
        require(ref, state)
    st = SqairStream(c, B, frames_per_step=S_, use_graph=False)
    st.step(obs, noise=nz)
    got = host(st.forecast(Fn, noise=fnoise))
    for k in EXACT:
        want = ref[k].numpy().astype(np.float32)
        assert np.array_equal(got[k], want), (k, differ(got[k], want))
    worst = {k: scaled(got[k], ref[k].numpy()) for k in CLOSE}
    print(case, "margin {:.4f}".format(mg), {k: "{:.1e}".format(v) for k, v in worst.items()}, "present", int(got["presence"].sum()))
    for k, e in worst.items():
        assert e <= ORACLE_GATE, (k, e)
    # the summaries of this forecast: the stream's weights are its running log-weight sums
    w = got["weights"].astype(np.float64)
    lw = st.log_weight_sum.cpu().numpy().astype(np.float64).reshape(B, K)
    want = np.exp(lw - lw.max(1, keepdims=True)) / np.exp(lw - lw.max(1, keepdims=True)).sum(1, keepdims=True)
    assert np.allclose(w, want, rtol=1e-5), ("weights", w, want)
    st.close()
    return got, ref


def filter_case(case, flags, B, TS, n_frames, frac, caller, edits=None, require=None):
    """SqairStream(resample="systematic") over n_frames frames against the fp64 particle filter of tests/smc_ref.py gathered through
    the device's own ancestors (tests/test_smc_oracle.py states what is compared and at which bars).  edits: names of
    tests/latent_regimes.EDITS applied to the parameters; require(outputs, step): a condition on the ORACLE filter's proposal of a
    step (what the case is meant to reach), checked before the device runs that step."""
    HW, GATE, REL = ORACLE_HW, ORACLE_GATE, ORACLE_REL
    F, P, obs, _ = setup(flags, B, n_frames, HW, 19, edits=edits)
    K = int(F.k_particles)
    R = B * K
    c = core(F, HW, P)
    if "n_what" in flags:
        assert c.lib is _capi.lib(_capi.WIDE_LIB_PATH), "the wide library was meant to serve this case"
    st = SqairStream(c, B, frames_per_step=TS, outputs=FILTER_OUTS, seed=41, resample="systematic", ess_frac=frac)
    pf = S.ParticleFilter(P, F, HW, B)
    rng = np.random.default_rng(7)
    steps = n_frames // TS
    reset_at, reset_lane = steps // 2, B - 1
    n = dict(went=0, moved=0, dec_checked=0, dec_skipped=0, anc_checked=0, anc_skipped=0)
    worst = dict(out=0.0, lw=0.0, ev=0.0, delta=0.0)
    for s in range(steps):
        fr = obs[s * TS:(s + 1) * TS]
        for attempt in range(DRAWS):   # the oracle's own presence margin decides; the device is not looked at
            nz = noise(F, rng, TS, R)
            prop = pf.propose(fr, nz)
            if float(presence_margins(prop[0], nz).min()) >= MARGIN:
                break
        else:
            raise AssertionError("no decision-stable noise draw in {} attempts at step {}".format(DRAWS, s))
        if require is not None:
            require(prop[0], s)
        lw0_ref, lz0_ref = pf.log_w.copy(), pf.log_z.copy()
        ref, rw = pf.commit(prop)
        lw0 = st.log_weight_sum.cpu().numpy()
        u_in = rng.uniform(size=B).astype(np.float32) if caller else None
        o = host(st.step(fr, noise=nz, uniforms=u_in))
        u = st.u.cpu().numpy()
        lw1, lz1 = st.log_weight_sum.cpu().numpy(), st.log_z.cpu().numpy()
        # the uniform: the caller's, or Philox keyed by the lane's frame counter after the step (the ORACLE's counter)
        if caller:
            assert np.array_equal(u, u_in), (s, u, u_in)
        else:
            want = S.smc_uniform(np.arange(B), pf.state.t.numpy()[::K], 41)
            assert np.array_equal(u, want), (s, u, want)
        # per-frame outputs
        for k in ("presence", "obj_id"):
            want = ref[k].numpy()
            assert np.array_equal(o[k].reshape(want.shape), want.astype(np.float32)), (s, k, differ(o[k].reshape(want.shape), want.astype(np.float32)))
        for k in ("what", "where", "presence_prob"):
            e = scaled(o[k], ref[k].numpy())
            worst["out"] = max(worst["out"], e)
            assert e <= GATE, (s, k, e)
        lw_ref = ref["log_weights_per_timestep"].numpy()
        e = float((np.abs(o["log_weights_per_timestep"] - lw_ref) / np.maximum(1.0, np.abs(lw_ref))).max())
        worst["lw"] = max(worst["lw"], e)
        assert e <= REL, (s, e)
        # the carried a_k (device: fp32 in frame order) and the evidence, relative to the largest of the value and the terms
        # summed into it (a sum of large terms that cancels carries their fp32 rounding, not its own)
        a_dev = accumulate(lw0, o["log_weights_per_timestep"]).astype(np.float64)
        a_scale = np.maximum.reduce([np.ones(R), np.abs(pf.a), np.abs(lw0_ref), np.abs(lw_ref).max(0)])
        e = float((np.abs(a_dev - pf.a) / a_scale).max())
        assert e <= REL, (s, "a_k", e)
        ev_scale = np.maximum.reduce([np.ones(B), np.abs(rw.log_evidence), np.abs(lz0_ref), np.abs(rw.w.m)])
        e = float((np.abs(o["log_evidence"] - rw.log_evidence) / ev_scale).max())
        worst["ev"] = max(worst["ev"], e)
        assert e <= REL, (s, "log_evidence", e, o["log_evidence"], rw.log_evidence)
        delta = np.abs(a_dev - pf.a).reshape(B, K).max(1)   # measured log-weight discrepancy per lane
        worst["delta"] = max(worst["delta"], float(delta.max()))
        # decisions on the oracle's ESS
        went = o["resampled"].astype(bool)
        for b in range(B):
            if frac == 1.0:
                want = True
            elif abs(rw.ess[b] - frac * K) <= (8 * delta[b] + 1e-5) * rw.ess[b]:
                n["dec_skipped"] += 1
                want = bool(went[b])
            else:
                n["dec_checked"] += 1
                want = bool(rw.ess[b] < frac * K)
            assert went[b] == want, (s, b, rw.ess[b], o["ess"][b])
            rows = slice(b * K, (b + 1) * K)
            anc = o["ancestors"][rows] - b * K
            if not went[b]:
                assert np.array_equal(anc, np.arange(K)), (s, b, anc)
                e = float((np.abs(lw1[rows] - pf.a[rows]) / a_scale[rows]).max())
                assert e <= REL, (s, b, "carried log_w", e)
                continue
            n["went"] += 1
            assert (lw1[rows] == 0).all(), (s, b, lw1[rows])
            assert abs(lz1[b] - rw.log_evidence[b]) <= REL * ev_scale[b], (s, b, lz1[b], rw.log_evidence[b], ev_scale[b])
            want_anc, c_, thr = S.systematic(rw.w.e[b], u[b])
            amb = (np.abs(c_[None, :] - thr[:, None]) <= 2 * delta[b] * rw.w.S[b]).any(1)
            n["anc_skipped"] += int(amb.sum())
            n["anc_checked"] += int((~amb).sum())
            assert np.array_equal(anc[~amb], want_anc[~amb]), (s, b, anc, want_anc)
            n["moved"] += int(not np.array_equal(anc, np.arange(K)))
        # the filter follows the device's map; a lane reset in mid-stream starts fresh on both
        src = o["ancestors"].astype(np.int64)
        pf.advance(src, went)
        if s == reset_at:
            st.reset([reset_lane])
            src2 = np.arange(R)
            src2[reset_lane * K:(reset_lane + 1) * K] = -1
            pf.state = pf.orc.gather_state(pf.state, src2)
            pf.reset([reset_lane])
    print(case, n, worst)
    if K > 1:
        assert n["went"] > 0 and n["moved"] > 0, n
        assert n["anc_checked"] > 0 and n["anc_skipped"] <= 0.1 * (n["anc_checked"] + n["anc_skipped"]), n
    else:
        assert n["went"] == steps * B, n
    assert n["dec_skipped"] <= max(1, 0.2 * n["dec_checked"]), n
    st.close()
    return n, worst


def stable_chunk(orc, frames, K, state, rng, F, R, T, grad):
    for _ in range(8):   # the oracle's own presence margin decides; the device is not looked at
        nz = noise(F, rng, T, R)
        if grad:
            target, out, st = tbptt_ref.chunk_target(orc, frames, nz, K, state)
        else:
            with torch.no_grad():
                target, out, st = tbptt_ref.chunk_target(orc, frames, nz, K, state)
        if float(presence_margins(out, nz).min()) >= MARGIN:
            return nz, target, out, st
    raise AssertionError("no decision-stable noise draw")


def chunk_two_case(flags, path, smc, require=None, edits=None):
    """Chunk 2 of a trained stream (imported rows, counters >= 1, present objects, one lane reset) against the fp64 oracle started
    from its own detached state.  require(out1, out2): a condition on the ORACLE's outputs of the two chunks (what the case is meant
    to reach), checked before the device runs chunk 2."""
    B, T, HW = 3, 3, ORACLE_HW
    F, obs, P = train_setup(flags, B, 2 * T, HW, 23, edits=edits)
    K = int(F.k_particles)
    R = B * K
    c = core(F, HW, P)
    if path:
        assert c.lib is _capi.lib(path), "the library at {} was meant to serve this case".format(path)
    tr = StreamTrainer(c, F, B, frames_per_step=T, use_graph=False, collective=False,
                       resample="systematic" if smc else None, outputs=("presence", "obj_id"))
    orc = O.SqairOracle(P, O.make_cfg(F, HW), torch.float64, requires_grad=True)
    rng = np.random.default_rng(11)
    # chunk 1: every row fresh, on both
    noise1, _, out1, st1 = stable_chunk(orc, obs[:T], K, None, rng, F, R, T, grad=False)
    tr.step(obs[:T], noise=noise1)
    torch.cuda.synchronize()
    for k in ("presence", "obj_id"):
        got, want = c.out[k].cpu().numpy(), out1[k].numpy().astype(np.float32)
        assert np.array_equal(got, want), ("chunk 1", k, differ(got, want))
    # chunk 2: imported rows (through the resampler's ancestors with SMC), one lane reset
    src = tr.ancestors.cpu().numpy().astype(np.int64) if smc else np.arange(R)
    tr.reset([B - 1])
    src[(B - 1) * K:] = -1
    st2 = orc.gather_state(st1, src)
    assert (st2.t.numpy()[:(B - 1) * K] >= 1).all(), ("imported counters", st2.t.numpy())
    noise2, target, out2, _ = stable_chunk(orc, obs[T:], K, st2, rng, F, R, T, grad=True)
    # present objects propagated at the chunk's first frame
    assert out2["prop_pres"][0].detach().numpy()[:(B - 1) * K].any(), "no present object is propagated into chunk 2"
    if require is not None:
        require(out1, out2)
    for p in orc.P.values():
        p.grad = None
    target.backward()
    tr.step(obs[T:], noise=noise2)
    torch.cuda.synchronize()
    for k in ("presence", "obj_id"):
        got, want = c.out[k].cpu().numpy(), out2[k].detach().numpy().astype(np.float32)
        assert np.array_equal(got, want), ("chunk 2", k, differ(got, want))
    report = []
    for name, g in c.grads_by_name().items():
        want = orc.P[name].grad
        g = g.cpu().numpy()
        want = np.zeros_like(g) if want is None else want.numpy().reshape(g.shape)
        report.append((name, float(np.abs(g - want).max()), float(np.abs(want).max())))
    names = {n for n, _, s in report if s > 0}
    for n in ("disc.step_prior_timestep_bias", "seq.temporal_init", "seq.prior_init"):
        assert any(m.startswith(n) for m in names), n
    check_report(report)
