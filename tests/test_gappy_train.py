"""-m gpu: training on gappy and ragged streams (include/sqair_hip.h: sqair_forward_train_carry_masked /
sqair_backward_carry_masked; StreamTrainer(missing=True).step(observed=...)).

1. a mask with every lane observed is the carried step: outputs and blob bit for bit, gradient to float-atomic order;
2. chunk 2 of a stream under a mixed mask -- a lane with a gap, a lane with a ragged tail, imported rows -- against the fp64
   reference of tests/gappy_train_ref.py, every parameter's gradient at the bars of tests/pass_cases.py;
3. a chunk without any observed lane: target 0, every gradient entry 0;
4. one lane observed in its first 2 of 4 frames: half the gradient of the 2-frame chunk;
5. the frames of unobserved lanes do not matter;
6. with the parameters held, masked chunked training is the masked SqairStream, and hands its state over;
7. one captured graph replays chunks with different masks and equals eager;
8. node counts.

Noise is picked on the REFERENCE's margins alone, and what a case is meant to reach is asserted on the reference before the HIP
path runs chunk 2."""
import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from sqair_amd.train import StreamTrainer
from tests import gappy_train_ref as GR
from tests.hip_util import MARGIN
from tests.pass_cases import TIGHT, check_report
from tests.stream_harness import (OUTS, chunks as _chunks, core, gclose, noise as _noise, train_setup, train_step)

pytestmark = pytest.mark.gpu

HW = (32, 40)
B, T = 3, 4
LSTM = dict(time_transition="LSTM", prior_transition="LSTM")
# lane 0 sees every frame, lane 1 has a gap of two frames and is observed again, lane 2's clip ends after two frames
MASK = np.array([[1, 1, 1], [1, 0, 1], [1, 0, 0], [1, 1, 0]], bool)
# prop_prior_step_bias = 1: a prior presence probability near 0.7, so that coasted frames drop objects and the score term of their
# presences is not vanishingly small (the default, 10, keeps every coasted object alive with probability 0.99995)
BASE = dict(n_steps_per_image=2, prop_prior_step_bias=1.0)
# name: (flags, library, SMC, core options, seed of the noise: the first, from 11 or from 1, whose draws meet reference_chunk_two's
# conditions -- found on the CPU, the device was not looked at)
CASES = {
    "gru": (dict(k_particles=3, **BASE), None, False, None, 11),
    "lstm": (dict(k_particles=3, **BASE, **LSTM), None, False, None, 11),
    "n_units_5": (dict(k_particles=3, n_units=5, **BASE), None, False, None, 11),
    "wide_n_what_64": (dict(k_particles=2, n_what=64, **BASE), _capi.WIDE_LIB_PATH, False, None, 11),
    "gru_smc": (dict(k_particles=3, **BASE), None, True, None, 11),
    "rw": (dict(k_particles=3, prop_prior_type="rw", **BASE), None, False, None, 16),
    "guided": (dict(k_particles=3, prop_prior_type="guided", rec_where_prior=True, **BASE), None, False, None, 10),
    "slot_chain": (dict(k_particles=3, **BASE), None, False, {"slot_chain": 1}, 11),
}
SMC_U = 0.37     # the resampler's uniform of every lane at the end of chunk 1


def _setup(flags, b, frames, seed=23):
    return train_setup(flags, b, frames, HW, seed)


def _core(F, P, options=None):
    return core(F, HW, P, options)


def _masks(n, b, t, seed=1):
    """n masks [t, b] with observed and unobserved entries in every one, frame 0 of the first observed."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        m = rng.uniform(size=(t, b)) < 0.6
        if m.any() and not m.all():
            out.append(m)
    return out


# ---- the reference side of test 2 (CPU only: tools and seed searches call it without a device) -------------------------------------
def _grads(orc, target):
    for p in orc.P.values():
        p.grad = None
    target.backward()
    return {n: (np.zeros(tuple(p.shape)) if p.grad is None else p.grad.numpy().copy()) for n, p in orc.P.items()}


def _stable(orc, frames, K, mask, state, rng, F, R):
    for _ in range(8):   # the oracle's own posterior and prior presence margins decide; the device is not looked at
        noise = _noise(F, rng, T, R)
        target, out, st = GR.chunk_target(orc, frames, noise, K, mask, state)
        if min(float(out["presence_margins"].min()), float(out["prior_margin"].min())) >= MARGIN:
            return noise, target, out, st
    raise AssertionError("no decision-stable noise draw")


def reference_chunk_one(case):
    flags, path, smc, options, seed = CASES[case]
    F, obs, P = _setup(flags, B, 2 * T)
    K = int(F.k_particles)
    orc = O.SqairOracle(P, O.make_cfg(F, HW), torch.float64, requires_grad=True)
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        noise1, _, out1, st1 = _stable(orc, obs[:T], K, np.ones((T, B), bool), None, rng, F, B * K)
    return dict(F=F, obs=obs, P=P, K=K, R=B * K, orc=orc, rng=rng, noise1=noise1, out1=out1, st1=st1)


def mid_drops(out, mask, K):
    """Coasted (frame, row)s of the reference that drop an object which is not the last present one of its row, others staying."""
    pres, ids = out["presence"].detach().numpy(), out["obj_id"].detach().numpy()
    n = 0
    for t in range(1, mask.shape[0]):
        for b in np.flatnonzero(~mask[t]):
            for r in range(b * K, (b + 1) * K):
                live = [i for i, p in zip(ids[t - 1, r], pres[t - 1, r]) if p > 0]
                kept = [i for i, p in zip(ids[t, r], pres[t, r]) if p > 0]
                n += int(any(i not in kept for i in live[:-1]) and len(kept) > 0)
    return n


def reference_chunk_two(ctx, src, flags):
    """Chunk 2 under MASK from the rows ``src`` of chunk 1's state: the stable noise, the reference's outputs and gradients, and the
    conditions on the reference alone."""
    orc, K, R, F, obs = ctx["orc"], ctx["K"], ctx["R"], ctx["F"], ctx["obs"]
    st2 = orc.gather_state(ctx["st1"], src)
    assert (st2.t.numpy()[2 * K:][np.asarray(src)[2 * K:] >= 0] >= 1).all() and (np.asarray(src)[2 * K:] >= 0).any()   # lane 2: imported rows
    noise2, target, out2, _ = _stable(orc, obs[T:], K, MASK, st2, ctx["rng"], F, R)
    # an object is alive in some row of lane 1 when its gap begins
    assert out2["presence"][0, K:2 * K].sum() > 0, "no object is present in lane 1 when its gap begins"
    if float(flags.get("prop_prior_step_bias", 10.0)) == 1.0:
        assert mid_drops(out2, MASK, K) > 0, "no coasted frame drops an object that is not the last one"
    grads = _grads(orc, target)
    # the test can see both new paths: without the score term, and with the coasted draws detached, some parameter of the prior
    # moves by at least 10 x the bar the device is held to
    gmax = max(float(np.abs(g).max()) for g in grads.values())
    for kw in (dict(score=False), dict(detach_draws=True)):
        other = _grads(orc, GR.chunk_target(orc, obs[T:], noise2, K, MASK, st2, **kw)[0])
        seen = [n for n in grads if n.startswith("prop.prior") and
                float(np.abs(other[n] - grads[n]).max()) >= 10.0 * TIGHT * max(float(np.abs(grads[n]).max()), 1e-4 * gmax)]
        assert seen, "the reference gradient does not depend on {} by 10 x the bar".format(kw)
    return noise2, out2, grads


# ---- 1. every lane observed is the carried step ------------------------------------------------------------------------------------
def test_all_observed_mask_is_the_carried_step():
    flags = dict(k_particles=3, n_steps_per_image=2)
    F, obs, P = _setup(flags, B, 2 * T)
    ta = StreamTrainer(_core(F, P), F, B, frames_per_step=T, use_graph=False, collective=False, outputs=OUTS, missing=True)
    tb = StreamTrainer(_core(F, P), F, B, frames_per_step=T, use_graph=False, collective=False, outputs=OUTS)
    for i, (fr, nz) in enumerate(_chunks(F, obs, B, T, 2)):
        a = train_step(ta, fr, noise=nz, observed=None if i == 0 else np.ones((T, B), bool))
        b = train_step(tb, fr, noise=nz)
        for k in ta.core.out:
            assert torch.equal(ta.core.out[k], tb.core.out[k]), (i, k)
        assert torch.equal(ta.state.view(torch.int32), tb.state.view(torch.int32)), i
        gclose(a, b, 1e-5)


# ---- 2. chunk 2 under a mixed mask against the fp64 reference ----------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_chunk_two_matches_the_fp64_reference(case):
    flags, path, smc, options, _ = CASES[case]
    ctx = reference_chunk_one(case)
    F, obs, K, R = ctx["F"], ctx["obs"], ctx["K"], ctx["R"]
    core = _core(F, ctx["P"], options)
    if path:
        assert core.lib is _capi.lib(path)
    tr = StreamTrainer(core, F, B, frames_per_step=T, use_graph=False, collective=False, resample="systematic" if smc else None,
                       outputs=("presence", "obj_id"), missing=True)
    tr.step(obs[:T], noise=ctx["noise1"], uniforms=np.full(B, SMC_U, np.float32) if smc else None)
    torch.cuda.synchronize()
    for k in ("presence", "obj_id"):
        assert np.array_equal(core.out[k].cpu().numpy(), ctx["out1"][k].numpy().astype(np.float32)), k
    src = tr.ancestors.cpu().numpy().astype(np.int64) if smc else np.arange(R)
    noise2, out2, grads = reference_chunk_two(ctx, src, flags)
    frames = obs[T:].copy()
    frames[~MASK] = np.nan            # never read
    tr.step(frames, noise=noise2, observed=MASK, uniforms=np.full(B, SMC_U, np.float32) if smc else None)
    torch.cuda.synchronize()
    if options:
        core.check_chain(train=True)
    for k in ("presence", "obj_id"):
        assert np.array_equal(core.out[k].cpu().numpy(), out2[k].detach().numpy().astype(np.float32)), k
    for k in ("log_weights_per_timestep", "discrete_log_prob"):
        got, want = core.out[k].cpu().numpy().astype(np.float64), out2[k].detach().numpy()
        rows = np.repeat(MASK, K, axis=1)
        assert float(np.abs(got - want).max()) <= 5e-4 * max(1.0, float(np.abs(want).max())), k
        if k == "log_weights_per_timestep":
            assert not got[~rows].any()
        else:   # the score term where the lane is observed later, an exact 0 in a ragged tail
            assert (got[1:3, K:2 * K] <= 0).all() and (got[1:3, K:2 * K] < 0).any() and not got[2:, 2 * K:].any()
    report = []
    for name, g in core.grads_by_name().items():
        g = g.cpu().numpy()
        want = grads[name].reshape(g.shape)
        report.append((name, float(np.abs(g - want).max()), float(np.abs(want).max())))
    names = {n for n, _, s in report if s > 0}
    assert any(m.startswith("prop.prior") for m in names)
    check_report(report)


# ---- 3. no lane observed -----------------------------------------------------------------------------------------------------------
def test_no_lane_observed_gives_target_zero_and_a_zero_gradient():
    flags = dict(k_particles=3, prop_prior_type="guided", **BASE)     # (guided: every route of the coasted adjoint is live)
    F, obs, P = _setup(flags, B, 2 * T)
    tr = StreamTrainer(_core(F, P), F, B, frames_per_step=T, use_graph=False, collective=False, outputs=OUTS, missing=True)
    (f1, n1), (f2, n2) = _chunks(F, obs, B, T, 2)
    g1 = train_step(tr, f1, noise=n1)
    assert np.abs(g1).max() > 0 and float(tr.core.out["presence"][-1].sum()) > 0       # objects enter the chunk
    g2 = train_step(tr, np.full_like(f2, np.nan), noise=n2, observed=np.zeros((T, B), bool))
    assert float(tr.core.scalars[2]) == 0.0                                            # vimco_target
    assert not tr.core.out["log_weights_per_timestep"].any() and not tr.core.out["discrete_log_prob"].any()
    assert float(tr.core.out["presence"].sum()) > 0                                     # ... and coast through it
    assert not g2.any()


# ---- 4. a ragged tail --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", ["gru", "lstm"])
def test_ragged_tail_is_the_short_chunk_scaled(cell):
    flags = dict(k_particles=3, **BASE, **(LSTM if cell == "lstm" else {}))
    F, obs, P = _setup(flags, 1, T)
    nz = _noise(F, np.random.default_rng(7), T, 3)
    ta = StreamTrainer(_core(F, P), F, 1, frames_per_step=T, use_graph=False, collective=False, missing=True)
    tb = StreamTrainer(_core(F, P), F, 1, frames_per_step=2, use_graph=False, collective=False)
    a = train_step(ta, obs, noise=nz, observed=np.array([[1], [1], [0], [0]], bool))
    b = train_step(tb, obs[:2], noise=nz[:2])
    assert float(tb.core.out["presence"].sum()) > 0
    gclose(a, 0.5 * b, 1e-5)


# ---- 5. the frames of unobserved lanes do not matter -------------------------------------------------------------------------------
def test_frames_of_unobserved_lanes_do_not_matter():
    flags = dict(k_particles=3, **BASE)
    F, obs, P = _setup(flags, B, 2 * T)
    ta = StreamTrainer(_core(F, P), F, B, frames_per_step=T, use_graph=False, collective=False, outputs=OUTS, missing=True)
    tb = StreamTrainer(_core(F, P), F, B, frames_per_step=T, use_graph=False, collective=False, outputs=OUTS, missing=True)
    for i, (fr, nz) in enumerate(_chunks(F, obs, B, T, 2)):
        mask = MASK if i else np.roll(MASK, 1, axis=1)
        other = fr.copy()
        other[~mask] = np.nan
        a = train_step(ta, fr, noise=nz, observed=mask)
        b = train_step(tb, other, noise=nz, observed=mask)
        for k in ta.core.out:
            assert torch.equal(ta.core.out[k], tb.core.out[k]), (i, k)
        assert torch.equal(ta.state.view(torch.int32), tb.state.view(torch.int32)), i
        assert np.isfinite(b).all()
        gclose(a, b, 1e-5)


# ---- 6. with the parameters held, masked chunked training is the masked stream -----------------------------------------------------
def test_masked_chunked_training_is_the_masked_stream_and_hands_over():
    flags = dict(k_particles=3, **BASE)
    F, obs, P = _setup(flags, B, 4 * T)
    chunks = _chunks(F, obs, B, T, 4)
    masks = _masks(4, B, T)
    tr = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False, use_graph=False, outputs=OUTS, missing=True)
    st = SqairStream(_core(F, P), B, frames_per_step=T, outputs=OUTS, use_graph=False, missing=True)
    coasted = 0
    for i, ((fr, nz), m) in enumerate(zip(chunks[:3], masks)):
        if i == 2:
            tr.reset([1])
            st.reset([1])
        train_step(tr, fr, noise=nz, observed=m)
        got = {k: tr.core.out[k].clone() for k in OUTS}
        want = st.step(fr, noise=nz, observed=m)
        torch.cuda.synchronize()
        for k in OUTS:
            assert torch.equal(got[k], want[k]), (i, k)
        coasted += int(got["presence"].cpu().numpy()[np.repeat(~m, int(F.k_particles), axis=1)].sum())
    assert coasted > 0                                              # objects were carried through unobserved frames
    assert torch.equal(tr.state.view(torch.int32), st.state.view(torch.int32))
    # hand-over: a masked stream on the trainer's core continues from its blob as the stream that saw every step
    st2 = SqairStream(tr.core, B, frames_per_step=T, outputs=OUTS, use_graph=False, state=tr.state, missing=True)
    a = st2.step(*chunks[3], observed=masks[3])
    b = st.step(*chunks[3], observed=masks[3])
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(st2.state.view(torch.int32), st.state.view(torch.int32))
    st2.close()
    st.close()


# ---- 7. one captured graph for every mask; 8. node counts --------------------------------------------------------------------------
@pytest.mark.parametrize("smc", [False, True])
def test_one_graph_replays_every_mask_and_node_budget(smc):
    flags = dict(k_particles=3, **BASE)
    F, obs, P = _setup(flags, B, 4 * T)
    chunks = _chunks(F, obs, B, T, 4)
    masks = [None] + _masks(3, B, T, seed=3)
    rs = "systematic" if smc else None
    tg = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False, resample=rs, missing=True)
    te = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False, resample=rs, missing=True, use_graph=False)
    keys = []
    for (fr, nz), m in zip(chunks, masks):
        u = np.full(B, SMC_U, np.float32) if smc else None
        a = train_step(tg, fr, noise=nz, uniforms=u, observed=m)      # chunk 0 runs eagerly and captures; chunks 1..3 replay
        b = train_step(te, fr, noise=nz, uniforms=u, observed=m)
        gclose(a, b, 1e-5)
        for k in tg.core.out:
            assert torch.equal(tg.core.out[k], te.core.out[k]), k
        assert torch.equal(tg.state.view(torch.int32), te.state.view(torch.int32))
        keys.append(tg.core._train_graph_key)
    assert all(k is keys[0] for k in keys)                        # captured once
    # the budget: T' + 1 kernel nodes more each way than the carried step, which itself is what it was
    tu = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False, resample=rs)
    with pytest.raises(ValueError, match="missing=True"):
        tu.step(chunks[0][0], noise=chunks[0][1], observed=masks[1])
    train_step(tu, chunks[0][0], noise=chunks[0][1], uniforms=np.full(B, SMC_U, np.float32) if smc else None)
    plain = _core(F, P)
    plain.bind(T, B, list(tu.core.out))
    plain.obs.copy_(torch.as_tensor(chunks[0][0]))
    with plain.on_stream():
        plain.grad_step()
    torch.cuda.synchronize()
    assert tu.core.train_graph_nodes == plain.train_graph_nodes + (3 if smc else 2)       # observed=None: today's count
    assert tg.core.train_graph_nodes == tu.core.train_graph_nodes + 2 * (T + 1)
