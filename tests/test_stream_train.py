"""-m gpu: training with a carried state (include/sqair_hip.h: SqairCarry; sqair_amd.train.StreamTrainer).

* a carried step with every row fresh is the plain training step (outputs bit for bit, gradient to float-atomic order), and its
  exported blob is the one an inference pass exports;
* chunk 2 of a stream (imported rows, counters >= 1, present objects, one lane reset) against the fp64 oracle started from its own
  detached state, with and without SMC;
* chunked training with the parameters held is streaming inference, bit for bit, and hands its state over to a SqairStream;
* SMC at ess_frac = 1: the ancestors of the inference stream, and the chunks' elbo_iwae sum to the log evidence;
* graph replay = eager over several chunks; node counts; the slot chain; two data-parallel shards."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from sqair_amd.train import StreamTrainer
from tests.stream_cases import ORACLE_HW as HW, chunk_two_case
from tests.stream_harness import OUTS, chunks as _chunks, core, gclose, noise as _noise, train_setup, train_step

pytestmark = pytest.mark.gpu

LSTM = dict(time_transition="LSTM", prior_transition="LSTM")


def _setup(flags, B, T, seed=19):
    return train_setup(flags, B, T, HW, seed)


def _core(F, P, options=None):
    return core(F, HW, P, options)


def test_fresh_carry_is_the_plain_step():
    F, obs, P = _setup(dict(k_particles=3, n_steps_per_image=3), B=2, T=3)
    core = _core(F, P)
    B, T, R = 2, 3, 2 * 3
    core.bind(T, B, ["log_weights_per_timestep", "discrete_log_prob", "what", "where", "presence", "obj_id"])
    core.obs.copy_(torch.as_tensor(obs))
    core.noise.copy_(torch.as_tensor(_noise(F, np.random.default_rng(3), T, R)).reshape(core.noise.shape))
    with core.on_stream():
        core.forward(train=True)
        g0 = core.backward().clone()
        o0 = {k: v.clone() for k, v in core.out.items()}
        nbytes = core.lib.sqair_state_bytes(core.handle, B)
        blob, blob_inf = (torch.full((nbytes // 4,), 7.0, device=core.device) for _ in range(2))
        carry = _capi.SqairCarry(state_in=None, state_out=blob.data_ptr(), src_rows=None, state_bytes=nbytes, B=B)
        core.forward_carry(carry)
        g1 = core.backward_carry(carry).clone()
        o1 = {k: v.clone() for k, v in core.out.items()}
    core.stream.synchronize()
    for k in o0:
        assert torch.equal(o0[k], o1[k]), k
    gclose(g1.cpu().numpy(), g0.cpu().numpy(), 1e-5)
    # the inference pass over the same frames and noise exports the same blob
    core.check(core.lib.sqair_set_state(core.handle, None, blob_inf.data_ptr(), None, nbytes, B), "sqair_set_state")
    with core.on_stream():
        core.forward()
    core.stream.synchronize()
    core.check(core.lib.sqair_set_state(core.handle, None, None, None, 0, 0), "sqair_set_state")
    assert torch.equal(blob, blob_inf)


# name: (flags, library, SMC)
ORACLE_CASES = {
    "gru": (dict(k_particles=3, n_steps_per_image=2), None, False),
    "lstm": (dict(k_particles=3, n_steps_per_image=2, **LSTM), None, False),
    "n_units_5": (dict(k_particles=3, n_steps_per_image=2, n_units=5), None, False),
    "wide_n_what_64": (dict(k_particles=2, n_steps_per_image=2, n_what=64), _capi.WIDE_LIB_PATH, False),
    "gru_smc": (dict(k_particles=3, n_steps_per_image=2), None, True),
}


@pytest.mark.parametrize("case", sorted(ORACLE_CASES))
def test_chunk_two_matches_the_fp64_oracle(case):
    chunk_two_case(*ORACLE_CASES[case])


def test_chunked_training_is_streaming_and_hands_over():
    flags = dict(k_particles=3, n_steps_per_image=3)
    B, T = 2, 2
    F, obs, P = _setup(flags, B, 4 * T)
    chunks = _chunks(F, obs, B, T, 4)
    tr = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False, outputs=OUTS)
    st = SqairStream(_core(F, P), B, frames_per_step=T, outputs=OUTS)
    for i, (fr, nz) in enumerate(chunks[:3]):
        if i == 2:
            tr.reset([1])
            st.reset([1])
        train_step(tr, fr, noise=nz)
        got = {k: tr.core.out[k].clone() for k in OUTS}
        want = st.step(fr, noise=nz)
        torch.cuda.synchronize()
        for k in OUTS:
            assert torch.equal(got[k], want[k]), (i, k)
    assert torch.equal(tr.state, st.state)
    # hand-over: a stream on the trainer's core continues from its blob as the stream that saw every frame
    st2 = SqairStream(tr.core, B, frames_per_step=T, outputs=OUTS, state=tr.state)
    a = st2.step(*chunks[3])
    b = st.step(*chunks[3])
    torch.cuda.synchronize()
    for k in OUTS:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(st2.state, st.state)
    st2.close()
    st.close()


def test_smc_ancestors_and_evidence():
    flags = dict(k_particles=4, n_steps_per_image=2)
    B, T, n = 3, 2, 4
    F, obs, P = _setup(flags, B, n * T)
    chunks = _chunks(F, obs, B, T, n)
    tr = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False, resample="systematic", outputs=OUTS)
    st = SqairStream(_core(F, P), B, frames_per_step=T, outputs=OUTS, resample="systematic", ess_frac=1.0)
    rng = np.random.default_rng(2)
    elbo = np.zeros(B)
    moved = 0
    for fr, nz in chunks:
        u = rng.uniform(size=B).astype(np.float32)
        train_step(tr, fr, noise=nz, uniforms=u)
        elbo += tr.core.elbo_iwae_per_example.cpu().numpy().astype(np.float64)
        anc = tr.ancestors.clone()
        want = st.step(fr, noise=nz, uniforms=u)
        torch.cuda.synchronize()
        assert torch.equal(anc, want["ancestors"])
        assert torch.equal(tr.log_evidence, want["log_evidence"])
        moved += int(not torch.equal(anc.cpu(), torch.arange(B * int(F.k_particles), dtype=torch.int32)))
        ev = tr.log_evidence.cpu().numpy().astype(np.float64)
        assert (np.abs(elbo - ev) <= 1e-5 * np.maximum(1.0, np.abs(ev))).all(), (elbo, ev)
    assert moved > 0
    st.close()


@pytest.mark.parametrize("smc", [False, True])
def test_graph_replay_equals_eager_and_node_budget(smc):
    flags = dict(k_particles=3, n_steps_per_image=3)
    B, T, n = 2, 2, 4
    F, obs, P = _setup(flags, B, n * T)
    chunks = _chunks(F, obs, B, T, n)
    rs = "systematic" if smc else None
    tg = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False, resample=rs)
    te = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False, resample=rs, use_graph=False)
    for i, (fr, nz) in enumerate(chunks):
        if i == 2:
            tg.reset([0])
            te.reset([0])
        u = np.full(B, 0.37, np.float32) if smc else None
        a = train_step(tg, fr, noise=nz, uniforms=u)
        b = train_step(te, fr, noise=nz, uniforms=u)
        gclose(a, b, 1e-5)
        assert torch.equal(tg.state, te.state), i
    # the plain step of the same shape and outputs, captured the same way
    plain = _core(F, P)
    plain.bind(T, B, list(tg.core.out))
    plain.obs.copy_(torch.as_tensor(chunks[0][0]))
    with plain.on_stream():
        plain.grad_step()
    torch.cuda.synchronize()
    assert tg.core.train_graph_nodes == plain.train_graph_nodes + (3 if smc else 2)


def test_slot_chain_carried_gradient():
    flags = dict(k_particles=3, n_steps_per_image=3)
    B, T, n = 2, 2, 2
    F, obs, P = _setup(flags, B, n * T)
    chunks = _chunks(F, obs, B, T, n)
    ta = StreamTrainer(_core(F, P, options={"slot_chain": 1}), F, B, frames_per_step=T, collective=False)
    tb = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False)
    for fr, nz in chunks:
        a = train_step(ta, fr, noise=nz)
        b = train_step(tb, fr, noise=nz)
        ta.core.check_chain(train=True)
        gclose(a, b, 1e-5)
        assert torch.equal(ta.state, tb.state)


def test_two_shards_average_to_the_full_batch():
    flags = dict(k_particles=3, n_steps_per_image=3)
    B, T, n = 4, 2, 2
    F, obs, P = _setup(flags, B, n * T)
    K = int(F.k_particles)
    chunks = _chunks(F, obs, B, T, n)
    full = StreamTrainer(_core(F, P), F, B, frames_per_step=T, collective=False)
    shards = [StreamTrainer(_core(F, P), F, B // 2, frames_per_step=T, collective=False) for _ in range(2)]
    for fr, nz in chunks:
        g = train_step(full, fr, noise=nz)
        gs = []
        for j, sh in enumerate(shards):
            lanes, rows = slice(j * B // 2, (j + 1) * B // 2), slice(j * B // 2 * K, (j + 1) * B // 2 * K)
            gs.append(train_step(sh, fr[:, lanes], noise=nz[:, rows]))
        gclose((gs[0] + gs[1]) / 2, g, 2e-4)
