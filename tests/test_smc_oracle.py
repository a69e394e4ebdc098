"""-m gpu: SqairStream(resample="systematic") against the fp64 particle filter of tests/smc_ref.py (the oracle with its state
carried, gathered through the device's own ancestors so that both runs stay on one trajectory).

Per step the noise is drawn on the ORACLE filter's presence margin (as hip_util.stable_noise does; the HIP result is never looked
at), then: presence and ids exactly; the per-frame outputs within the live-oracle gate (5e-4 of max(1, |value|)); the per-frame log
weights, the carried ones and log_evidence within 1e-4 relative (the north-star bar; relative to the largest of the value
and the terms summed into it); the decisions and the device's ancestors
against the fp64 resampler run on the ORACLE's weights with the device's uniform, skipping only what the measured log-weight
discrepancy delta allows (|ESS - ess_frac K| within 8 delta ESS; |c_i - thr| <= 2 delta S).  A lane is reset in mid-stream, and
resampling must happen."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.data import make_sequences, to_float
from sqair_amd.flags import make_flags
from sqair_amd.model import SqairCore
from sqair_amd.stream import SqairStream
from tests import smc_ref as S
from tests.hip_util import MARGIN, draw_noise, params32, presence_margins

pytestmark = pytest.mark.gpu

OUTS = ("what", "where", "presence", "obj_id", "presence_prob", "log_weights_per_timestep")
GATE = 5e-4          # live-oracle gate (scaled absolute error) of the per-frame outputs
REL = 1e-4           # north-star bar: log weights and evidence (relative to max(1, the value, the terms summed into it))
DRAWS = 6            # noise draws per step before giving up on a decision-stable one
HW = (32, 40)
LSTM = dict(time_transition="LSTM", prior_transition="LSTM")

# name: (flags, B, frames_per_step, frames, ess_frac, caller uniforms)
CASES = {
    "gru": (dict(k_particles=4, n_steps_per_image=2), 3, 1, 10, 0.5, False),
    "lstm": (dict(k_particles=4, n_steps_per_image=2, **LSTM), 3, 1, 10, 1.0, True),
    "gru_3_frames_per_step": (dict(k_particles=4, n_steps_per_image=2), 2, 3, 12, 0.5, False),
    "lstm_3_frames_per_step": (dict(k_particles=3, n_steps_per_image=2, **LSTM), 2, 3, 12, 1.0, False),
    "k1": (dict(k_particles=1, n_steps_per_image=2), 4, 1, 10, 1.0, False),
    "k65": (dict(k_particles=65, n_steps_per_image=1), 1, 1, 10, 0.5, True),
    "wide_n_what_64": (dict(k_particles=3, n_steps_per_image=2, n_what=64), 2, 1, 10, 1.0, False),
}


def _scaled(got, want):
    got = np.asarray(got, np.float64).reshape(want.shape)
    return float(np.abs(got - want).max() / max(1.0, float(np.abs(want).max())))


@pytest.mark.parametrize("case", sorted(CASES))
def test_stream_matches_the_fp64_particle_filter(case):
    _filter_case(case, *CASES[case])


def _filter_case(case, flags, B, TS, frames, frac, caller, edits=None, require=None):
    """edits: names of tests/latent_regimes.EDITS applied to the parameters; require(outputs, step): a condition on the ORACLE
    filter's proposal of a step (what the case is meant to reach), checked before the device runs that step."""
    F = make_flags(**flags)
    K, N, nzw = int(F.k_particles), int(F.n_steps_per_image), 4 + int(F.n_what) + 1
    R = B * K
    obs = to_float(make_sequences(B, T=frames, canvas=HW, seed=19)["imgs"])
    P = params32(F, HW, 3, 0.05, obs.mean((0, 1)))
    if edits:   # names of tests/latent_regimes.EDITS (tests/test_regime_paths.py)
        from tests import latent_regimes
        P = latent_regimes.apply_edits(P, F, edits)
    core = SqairCore(F, HW)
    core.set_params(P)
    if "n_what" in flags:
        assert core.lib is _capi.lib(_capi.WIDE_LIB_PATH)
    st = SqairStream(core, B, frames_per_step=TS, outputs=OUTS, seed=41, resample="systematic", ess_frac=frac)
    pf = S.ParticleFilter(P, F, HW, B)
    rng = np.random.default_rng(7)
    steps = frames // TS
    reset_at, reset_lane = steps // 2, B - 1
    n = dict(went=0, moved=0, dec_checked=0, dec_skipped=0, anc_checked=0, anc_skipped=0)
    worst = dict(out=0.0, lw=0.0, ev=0.0, delta=0.0)
    for s in range(steps):
        fr = obs[s * TS:(s + 1) * TS]
        for attempt in range(DRAWS):   # the oracle's own presence margin decides; the device is not looked at
            noise = draw_noise(rng, TS, R, N, nzw)
            prop = pf.propose(fr, noise)
            if float(presence_margins(prop[0], noise).min()) >= MARGIN:
                break
        else:
            raise AssertionError("no decision-stable noise draw in {} attempts at step {}".format(DRAWS, s))
        if require is not None:
            require(prop[0], s)
        lw0_ref, lz0_ref = pf.log_w.copy(), pf.log_z.copy()
        ref, rw = pf.commit(prop)
        lw0 = st.log_weight_sum.cpu().numpy()
        u_in = rng.uniform(size=B).astype(np.float32) if caller else None
        out = st.step(fr, noise=noise, uniforms=u_in)
        torch.cuda.synchronize()
        o = {k: v.cpu().numpy() for k, v in out.items()}
        u = st.u.cpu().numpy()
        lw1, lz1 = st.log_weight_sum.cpu().numpy(), st.log_z.cpu().numpy()
        # the uniform: the caller's, or Philox keyed by the lane's frame counter after the step (the ORACLE's counter)
        if caller:
            assert np.array_equal(u, u_in)
        else:
            assert np.array_equal(u, S.smc_uniform(np.arange(B), pf.state.t.numpy()[::K], 41)), s
        # per-frame outputs
        for k in ("presence", "obj_id"):
            want = ref[k].numpy()
            assert np.array_equal(o[k].reshape(want.shape), want.astype(np.float32)), (s, k)
        for k in ("what", "where", "presence_prob"):
            e = _scaled(o[k], ref[k].numpy())
            worst["out"] = max(worst["out"], e)
            assert e <= GATE, (s, k, e)
        lw_ref = ref["log_weights_per_timestep"].numpy()
        e = float((np.abs(o["log_weights_per_timestep"] - lw_ref) / np.maximum(1.0, np.abs(lw_ref))).max())
        worst["lw"] = max(worst["lw"], e)
        assert e <= REL, (s, e)
        # the carried a_k (device: fp32 in frame order) and the evidence, relative to the largest of the value and the terms
        # summed into it (a sum of large terms that cancels carries their fp32 rounding, not its own)
        a_dev = S.accumulate(lw0, o["log_weights_per_timestep"]).astype(np.float64)
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
                assert np.array_equal(anc, np.arange(K))
                e = float((np.abs(lw1[rows] - pf.a[rows]) / a_scale[rows]).max())
                assert e <= REL, (s, b, "carried log_w", e)
                continue
            n["went"] += 1
            assert (lw1[rows] == 0).all()
            assert abs(lz1[b] - rw.log_evidence[b]) <= REL * ev_scale[b]
            want_anc, c, thr = S.systematic(rw.w.e[b], u[b])
            amb = (np.abs(c[None, :] - thr[:, None]) <= 2 * delta[b] * rw.w.S[b]).any(1)
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
