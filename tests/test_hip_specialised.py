"""The specialised instantiations of the slot loop's crops and of the compaction (csrc/sqair_glue.h: sq_spec_ok; option
"specialised", default on) against the generic ones: the same expressions in the same order on the same operands, with the shipped
dimensions and the launch's mode as compile-time constants -- every output bit for bit."""
import numpy as np
import pytest
import torch

from sqair_amd.data import make_sequences, to_float
from sqair_amd.flags import make_flags
from tests.hip_util import draw_noise, params32

from tests.pass_cases import spec_launches

pytestmark = pytest.mark.gpu


def _outputs(core):
    out = {k: v.detach().cpu().numpy().copy() for k, v in core.out.items()}
    out["log_weights"] = core.log_weights.cpu().numpy().copy()
    return out


# B, K, N, T, frame, flags, takes the specialised path
CASES = [
    (32, 5, 4, 3, (50, 50), dict(), True),                       # the cfg-2 rows: 160 particle rows
    (5, 3, 4, 2, (50, 50), dict(), True),                        # the shipped dimensions, 15 rows (rows not spread over the XCDs)
    (32, 5, 4, 3, (50, 50), dict(n_what=10), False),             # another record width: generic
    (32, 5, 4, 3, (37, 41), dict(), False),                      # another frame (and H W not a multiple of 4): generic
    (4, 2, 6, 2, (50, 50), dict(), False),                       # six slots (the cfg-4 family): generic
]


@pytest.mark.parametrize("B,K,N,T,hw,flags,takes_spec", CASES, ids=["cfg2_rows", "15_rows", "n_what_10", "frame_37x41", "six_slots"])
def test_specialised_kernels_are_bit_identical_to_the_generic_ones(B, K, N, T, hw, flags, takes_spec):
    from sqair_amd.model import Model, SqairCore
    F = make_flags(k_particles=K, n_steps_per_image=N, **flags)
    d = make_sequences(B, T=T, canvas=hw, seed=17)
    obs = to_float(d["imgs"])
    P = params32(F, hw, 3, 0.05, obs.mean((0, 1)))
    noise = draw_noise(np.random.default_rng(11), T, B * K, N, 4 + int(F.n_what) + 1)

    def make(spec):
        core = SqairCore(F, hw, options={"specialised": int(spec)})
        core.set_params(P)
        return core, Model(obs, None, core, K, presence=d["nums"])

    def run_inference(spec, use_graph):
        core, m = make(spec)
        n0 = spec_launches()
        m.run(noise=noise, use_graph=use_graph)
        torch.cuda.synchronize()
        return _outputs(core), spec_launches() - n0, (core.lib.sqair_graph_nodes(core.handle) if use_graph else 0)

    def run_training(spec):
        # the training-mode forward pass (tape kept) eager, then again inside ONE graph replay of a gradient evaluation (forward
        # with tape + targets + backward).  The backward pass accumulates with atomics, so the gradient itself is not compared
        # bit for bit: what the replayed forward pass left in the outputs is.
        core, m = make(spec)
        n0 = spec_launches()
        with core.on_stream():
            core.noise.copy_(torch.as_tensor(noise).reshape(core.noise.shape))
            core.forward(train=True)
            core.stream.synchronize()
            eager = _outputs(core)
            n_fwd = spec_launches() - n0
            g = core.grad_step(use_graph=True).clone()
            core.stream.synchronize()
            replay = _outputs(core)
        assert bool(torch.isfinite(g).all())
        return eager, n_fwd, replay

    ref, n_off, _ = run_inference(False, False)
    assert n_off == 0, "option specialised = 0 must launch generic instantiations only"
    assert float(ref["presence"].sum()) > 0
    nodes = {}
    for use_graph in (False, True):
        got, n_on, nodes[use_graph] = run_inference(True, use_graph)
        # per frame: 1 + 2 N crops, 1 compaction
        assert n_on == (T * (1 + 2 * N + 1) if takes_spec else 0), (n_on, use_graph)
        assert set(got) == set(ref)
        for k, v in ref.items():
            assert np.array_equal(v, got[k], equal_nan=True), (k, use_graph)
    _, _, nodes_off = run_inference(False, True)
    assert nodes[True] == nodes_off, "an instantiation replaces a launch one for one"

    tref, tn_off, tref_replay = run_training(False)
    tgot, tn_on, tgot_replay = run_training(True)
    assert tn_off == 0
    assert tn_on == (T * (1 + 2 * N + 1) if takes_spec else 0), tn_on
    for k, v in tref.items():
        assert np.array_equal(v, tgot[k], equal_nan=True), (k, "train")
        assert np.array_equal(v, tgot_replay[k], equal_nan=True), (k, "train, graph replay")
        assert np.array_equal(v, tref_replay[k], equal_nan=True), (k, "train, graph replay, generic")
        if k in ref:
            assert np.array_equal(v, ref[k], equal_nan=True), (k, "train vs inference")


def test_specialised_is_a_documented_option_and_unknown_names_are_refused():
    from sqair_amd.model import SqairCore
    core = SqairCore(make_flags(), (50, 50))
    assert core.lib.sqair_set_option(core.handle, b"specialised", 0) == 0
    assert core.lib.sqair_set_option(core.handle, b"specialised", 1) == 0
    assert core.lib.sqair_set_option(core.handle, b"specialized_", 1) == -2
