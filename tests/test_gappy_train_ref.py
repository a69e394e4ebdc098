"""No GPU: the fp64 reference of a masked carried training chunk (tests/gappy_train_ref.py) against the pieces it restates --
every lane observed is tbptt_ref's chunk target, value and gradient; its outputs are coast_ref's on a mixed mask -- and the two
consequences the header states: no lane observed gives target 0 and a zero gradient, a lane observed only in its first s frames
gives s / T' times the gradient of the s-frame chunk."""
import numpy as np
import torch

from oracle import sqair_oracle as O
from sqair_amd.data import make_sequences, to_float
from sqair_amd.flags import make_flags
from tests import gappy_train_ref as GR
from tests import tbptt_ref as TR
from tests.coast_ref import coast_ref
from tests.hip_util import draw_noise, params32

HW, B, K, N, T = (32, 40), 2, 2, 2, 4
DT = torch.float64


def _setup(b=B, **flags):
    F = make_flags(k_particles=K, n_steps_per_image=N, **flags)
    obs = to_float(make_sequences(b, T=2 * T, canvas=HW, n_objects=(1, 2), obj_size=10, seed=23)["imgs"])
    P = params32(F, HW, 3, 0.05, obs.mean((0, 1)))
    orc = O.SqairOracle(P, O.make_cfg(F, HW), DT, requires_grad=True)
    rng = np.random.default_rng(29)
    noise = [draw_noise(rng, T, b * K, N, 4 + int(F.n_what) + 1) for _ in range(2)]
    return orc, obs, noise


def _grads(orc, target):
    for p in orc.P.values():
        p.grad = None
    target.backward()
    return {n: (torch.zeros_like(p) if p.grad is None else p.grad.clone()) for n, p in orc.P.items()}


def _chunk_one_state(orc, obs, noise):
    """The state after chunk 1 (objects in it, counters T), as constants."""
    with torch.no_grad():
        _, out, st = TR.chunk_target(orc, obs[:T], noise, K)
    assert float(st.z[2].sum()) > 0
    return st


def test_every_lane_observed_is_the_carried_chunk():
    orc, obs, noise = _setup()
    for state in (None, _chunk_one_state(orc, obs, noise[0])):
        want, wo, ws = TR.chunk_target(orc, obs[T:], noise[1], K, state)
        gw = _grads(orc, want)
        got, go, gs = GR.chunk_target(orc, obs[T:], noise[1], K, np.ones((T, B), bool), state)
        gg = _grads(orc, got)
        assert abs(float(got.detach()) - float(want.detach())) <= 1e-12 * abs(float(want.detach()))
        scale = max(float(v.abs().max()) for v in gw.values())
        assert scale > 0
        for n in gw:
            assert float((gg[n] - gw[n]).abs().max()) <= 1e-10 * scale, n
        for n in wo:
            if not n.startswith("_"):
                assert torch.allclose(go[n], wo[n], rtol=0.0, atol=1e-12), n
        assert torch.equal(gs.t, ws.t)


def test_outputs_are_coast_refs_on_a_mixed_mask():
    orc, obs, noise = _setup()
    state = _chunk_one_state(orc, obs, noise[0])
    mask = np.array([[1, 1], [0, 1], [1, 0], [1, 0]], bool)       # lane 0: a gap; lane 1: a ragged tail
    with torch.no_grad():
        _, got, gs = GR.chunk_target(orc, obs[T:], noise[1], K, mask, state)
        tiled = O.tile_input_for_iwae(torch.as_tensor(obs[T:], dtype=DT), K)
        want, ws = coast_ref(orc, TR.detach_state(state), tiled, noise[1], mask)
    score = np.repeat(GR.later_observed(mask) & ~mask, K, axis=1)    # coasted rows that keep their score term
    assert score.sum() == K and score[1, :K].all()
    for n, v in want.items():
        if n == "discrete_log_prob":
            assert torch.equal(got[n][~torch.as_tensor(score)], v[~torch.as_tensor(score)])
            s = GR.score_term(got["presence"][1, :K], got["presence_logit"][1, :K])
            assert torch.equal(got[n][1, :K], s) and bool((s < 0).all())
        else:
            assert np.array_equal(np.asarray(got[n]), np.asarray(v)), n
    for a, b in zip(gs.z + (gs.temporal, gs.prior, gs.prev_ids, gs.last_id), ws.z + (ws.temporal, ws.prior, ws.prev_ids, ws.last_id)):
        assert torch.equal(a, b)


def test_no_lane_observed_gives_target_zero_and_a_zero_gradient():
    orc, obs, noise = _setup()
    state = _chunk_one_state(orc, obs, noise[0])
    frames = np.full_like(obs[T:], np.nan)                          # never read
    target, out, _ = GR.chunk_target(orc, frames, noise[1], K, np.zeros((T, B), bool), state)
    assert float(target.detach()) == 0.0
    assert float(out["presence"].sum()) > 0                         # objects coast through the chunk
    assert not out["discrete_log_prob"].any() and not out["log_weights_per_timestep"].any()
    for n, g in _grads(orc, target).items():
        assert not g.any(), n


def test_ragged_identity():
    """One lane observed in its first s of T' frames: s / T' times the gradient of the s-frame chunk on the same frames and noise."""
    orc, obs, noise = _setup(b=1)
    state = _chunk_one_state(orc, obs, noise[0])
    s = 2
    mask = np.array([[1], [1], [0], [0]], bool)
    full, _, _ = GR.chunk_target(orc, obs[T:], noise[1], K, mask, state)
    gf = _grads(orc, full)
    short, _, _ = TR.chunk_target(orc, obs[T:T + s], noise[1][:s], K, state)
    gs = _grads(orc, short)
    assert abs(float(full.detach()) - float(short.detach()) * s / T) <= 1e-12 * abs(float(short.detach()))
    scale = max(float(v.abs().max()) for v in gs.values())
    assert scale > 0
    for n in gs:
        assert float((gf[n] - gs[n] * s / T).abs().max()) <= 1e-10 * scale, n
