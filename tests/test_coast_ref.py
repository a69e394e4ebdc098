"""No GPU: the fp64 reference of the missing-frame steps (tests/coast_ref.py) against the pieces it restates -- every lane observed is
the oracle's sequence, no lane observed is the forecast's rollout -- and a hand-built coasted frame that drops an object which is
not the last one: ids, prior and temporal states move to the right slots."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import sqair_oracle as O
from sqair_amd.data import make_sequences, to_float
from sqair_amd.flags import make_flags
from tests.coast_ref import COASTED, coast_ref, prior_frame
from tests.forecast_ref import forecast_ref
from tests.hip_util import draw_noise, params32

HW, B, K, N, T = (32, 40), 2, 2, 3, 3
DT = torch.float64


def _setup(**flags):
    F = make_flags(k_particles=K, n_steps_per_image=N, **flags)
    obs = to_float(make_sequences(B, T=T, canvas=HW, seed=19)["imgs"])
    P = params32(F, HW, 3, 0.05, obs.mean((0, 1)))
    orc = O.SqairOracle(P, O.make_cfg(F, HW), DT)
    tiled = O.tile_input_for_iwae(torch.as_tensor(obs, dtype=DT), K)
    noise = draw_noise(np.random.default_rng(23), T, B * K, N, 4 + int(F.n_what) + 1)
    return orc, tiled, noise


def _same(a, b):
    return torch.allclose(torch.as_tensor(a), torch.as_tensor(b), rtol=0.0, atol=1e-12)


def test_every_lane_observed_is_the_oracles_sequence():
    orc, tiled, noise = _setup()
    with torch.no_grad():
        want, ws = orc.sequence(tiled, torch.as_tensor(noise, dtype=DT), state=orc.initial_state(B * K), return_state=True)
    got, gs = coast_ref(orc, orc.initial_state(B * K), tiled, noise, np.ones((T, B), bool))
    names = [n for n in want if not n.startswith("_")]
    assert len(names) == 38
    for n in names:
        assert _same(got[n], want[n]), n
    for a, b in zip(gs.z + (gs.temporal, gs.prior, gs.prev_ids, gs.last_id), ws.z + (ws.temporal, ws.prior, ws.prev_ids, ws.last_id)):
        assert _same(a, b)
    assert torch.equal(gs.t, ws.t)
    assert (got["prior_margin"] == 1.0).all() and (got["presence_margins"] <= 1.0).all()


def test_no_lane_observed_is_the_forecast():
    orc, tiled, noise = _setup()
    with torch.no_grad():   # a state with objects in it: the oracle after the clip
        _, state = orc.sequence(tiled, torch.as_tensor(noise, dtype=DT), state=orc.initial_state(B * K), return_state=True)
    assert float(state.z[2].sum()) > 0
    fnoise = draw_noise(np.random.default_rng(5), 4, B * K, N, noise.shape[-1])
    fnoise[..., 0, :, -1] *= 0.9999   # (below the prior's probability: the objects live on)
    want = forecast_ref(orc, state, fnoise)
    got, gs = coast_ref(orc, state, np.full((4, B * K) + HW, np.nan), fnoise, np.zeros((4, B), bool))
    for n in COASTED:
        assert _same(got[n], want[n]), n
    assert float(want["presence"].sum()) > 0
    z, prior, prev_ids, last_id = want["_final"]
    for a, b in zip(gs.z + (gs.prior, gs.prev_ids, gs.last_id), z + (prior, prev_ids, last_id)):
        assert _same(a, b)
    assert torch.equal(gs.t, state.t + 4)
    # everything the posterior path would have written is zero, the log weight among them; the counts are the coasted records'
    for n, v in got.items():
        if n in COASTED or n in ("presence_margins", "prior_margin"):
            continue
        if n in ("num_prop_steps_per_sample", "num_steps_per_sample"):
            assert torch.equal(v, got["presence"].sum(-1)), n
        elif n == "prop_pres":
            assert torch.equal(v, got["presence"]), n
        else:
            assert not v.any(), n
    assert (got["presence_margins"] == 1.0).all()


def test_a_coasted_frame_that_drops_an_object_in_the_middle():
    orc, _, _ = _setup(prop_prior_step_bias=2.0)   # (a prior presence probability well inside (0, 0.999))
    c = orc.cfg
    R, nw = 2, c.n_what
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=DT)
    tw, pw = orc.initial_temporal_state().shape[-1], orc.initial_prior_state().shape[-1]
    state = SimpleNamespace(z=(rnd(R, N, nw), 0.3 * rnd(R, N, 4), torch.ones(R, N, 1, dtype=DT), torch.full((R, N, 1), 3.0, dtype=DT)),
                            temporal=rnd(R, N, tw), prior=0.1 * rnd(R, N, pw),
                            prev_ids=torch.tensor([[4.0, 7.0, 9.0], [0.0, 1.0, 2.0]], dtype=DT)[..., None],
                            last_id=torch.tensor([[11.0], [2.0]], dtype=DT), t=torch.tensor([5, 8]))
    eps = rnd(R, N, 4 + nw + 1)
    eps[..., -1] = 0.0
    eps[:, 1, -1] = 0.999      # the middle object goes, the others stay
    with torch.no_grad():
        stats, prior_new = orc.propagate_prior(state.z, state.prior)
        out, new = prior_frame(orc, state, eps)
    prob = torch.sigmoid(stats[4])
    assert float(prob.min()) > 0.0 and float(prob.max()) < 0.999
    order = [0, 2, 1]          # present first, stable; the dropped slot after them
    assert torch.equal(out["presence"], torch.tensor([[1.0, 1.0, 0.0]] * R, dtype=DT))
    assert torch.equal(out["obj_id"], torch.tensor([[4.0, 9.0, -1.0], [0.0, 2.0, -1.0]], dtype=DT))
    assert torch.equal(new.prev_ids.squeeze(-1), out["obj_id"])
    assert torch.equal(new.last_id, state.last_id)                       # nothing discovered: last_id does not move
    assert torch.equal(new.temporal, state.temporal[:, order])            # held, and carried with its slot
    assert torch.equal(new.prior, prior_new[:, order])                    # the prior cell's NEW state, carried with its slot
    assert torch.equal(new.t, state.t + 1)
    assert torch.equal(new.z[3], stats[4][:, order])                      # the record keeps the prior logit
    what = stats[2] + stats[3] * eps[..., 4:4 + nw]
    assert torch.equal(out["what"], what[:, order]) and torch.equal(new.z[0], out["what"])
