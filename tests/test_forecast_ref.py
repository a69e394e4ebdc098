"""No GPU: a self-check of the test helper tests/forecast_ref.py, not coverage of the forecast itself (tests/test_forecast.py and
tests/test_forecast_host.py call the library).  The fp64 rollout the device forecast is compared with must be the reference's
generation mode; here it is checked against the oracle's own restatement of that mode."""
import pytest

from sqair_amd.flags import make_flags


@pytest.mark.parametrize("prop_prior_type", ["rnn", "rw"])
def test_fp64_reference_is_the_oracles_generation_mode(prop_prior_type):
    """Reference self-check: tests/forecast_ref.py against the oracle's own generation mode (sample_from_prior,
    generate_after = t0): started from the oracle's state after frame t0 with the generation draws of the later frames, it gives
    those frames' objects and canvases.
    (rw: the first generated frame only -- later ones read the posterior logit there and the prior logit in a forecast.)"""
    import numpy as np
    import torch
    from oracle import sqair_oracle as O
    from sqair_amd.data import make_sequences, to_float
    from tests.forecast_ref import forecast_ref
    from tests.hip_util import draw_noise, params32

    hw, B, T, t0 = (32, 40), 2, 5, 2
    flags = dict(k_particles=2, n_steps_per_image=2, prop_prior_type=prop_prior_type)
    F = make_flags(**flags)
    Fg = make_flags(sample_from_prior=True, generate_after=t0, **flags)
    K, N, nzw = 2, 2, 4 + int(F.n_what) + 1
    obs = to_float(make_sequences(B, T=T, canvas=hw, seed=5)["imgs"])
    P = params32(F, hw, 3, 0.05, obs.mean((0, 1)))
    rng = np.random.default_rng(3)
    noise, gen = draw_noise(rng, T, B * K, N, nzw), draw_noise(rng, T, B * K, N, nzw)
    gen[..., 0, :, -1] = rng.uniform(0.0, 0.3, size=gen[..., 0, :, -1].shape)   # (objects that survive a few frames)
    noise, gen = torch.as_tensor(noise, dtype=torch.float64), torch.as_tensor(gen, dtype=torch.float64)
    tiled = O.tile_input_for_iwae(torch.as_tensor(obs, dtype=torch.float64), K)
    with torch.no_grad():
        whole = O.SqairOracle(P, O.make_cfg(Fg, hw)).sequence(tiled, noise, gen_noise=gen)
        orc = O.SqairOracle(P, O.make_cfg(F, hw))
        _, state = orc.sequence(tiled[:t0 + 1], noise[:t0 + 1], state=orc.initial_state(B * K), return_state=True)
    ref = forecast_ref(orc, state, gen[t0 + 1:])
    frames = T - t0 - 1 if prop_prior_type == "rnn" else 1
    for f in range(frames):
        t = t0 + 1 + f
        assert torch.equal(ref["presence"][f], whole["presence"][t]), f
        assert torch.equal(ref["obj_id"][f], whole["obj_id"][t]), f
        for n in ("what", "where", "canvas", "glimpse"):
            assert torch.allclose(ref[n][f], whole[n][t], atol=1e-12, rtol=0), (f, n)
    assert float(ref["presence"].sum()) > 0   # (the comparison saw objects)
