"""-m gpu: the device Philox4x32-10 generator (sqair_fill_noise, k_fill_noise in sqair_train.hip) against its NumPy restatement
(tests/smc_ref.py, pinned to the Random123 known answers by tests/test_smc_ref.py).

Every u (the presence Bernoullis' uniforms, 24 bits) must match bit for bit; every eps (Box-Muller) to 1e-5 absolute: the device's
logf / sqrtf / cosf are within a few ulps, |eps| < 6 and the restatement already uses the device's fp32 2 pi * u2, so the fp32
error is ~1e-6.  A wrong round constant, counter word or key word changes every value."""
import numpy as np
import pytest
import torch

from sqair_amd.flags import make_flags
from sqair_amd.model import SqairCore
from sqair_amd.stream import SqairStream
from tests import smc_ref as S

pytestmark = pytest.mark.gpu

HW = (32, 40)
EPS_TOL = 1e-5


def _check(noise, want):
    got = noise.detach().cpu().numpy().reshape(want.shape)
    u_got, u_want = got[..., -1], want[..., -1].astype(np.float32)
    assert np.array_equal(u_got, u_want), np.argwhere(u_got != u_want)[:4]
    err = float(np.abs(got[..., :-1].astype(np.float64) - want[..., :-1]).max())
    assert err <= EPS_TOL, err
    return err


# (T, B, global_B, b0, seed, steps)
CASES = {
    "one_frame": (1, 4, 4, 0, 7, (3,)),
    "frames_3": (3, 2, 2, 0, 123, (0,)),
    "sharded": (2, 3, 8, 5, 7, (3,)),
    "two_steps": (2, 4, 4, 0, 99, (0, 1)),
    "seed_above_2_32": (2, 2, 6, 1, (1 << 33) + 12345, (1 << 32) + 7,),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_fill_noise_matches_the_restatement(case):
    T, B, gB, b0, seed, steps = CASES[case]
    steps = steps if isinstance(steps, tuple) else (steps,)
    F = make_flags(k_particles=3, n_steps_per_image=3)
    K, N, nw = 3, 3, int(F.n_what)
    core = SqairCore(F, HW)
    core.bind(T, B, "minimal")
    seen = []
    for step in steps:
        core.draw_noise(seed=seed, step=step, global_batch=gB, b0=b0)
        torch.cuda.synchronize()
        want = S.fill_noise(T, B, K, N, nw, seed=seed, step=step, global_B=gB, b0=b0)
        _check(core.noise, want)
        seen.append(core.noise.cpu().numpy().copy())
    if len(seen) == 2:
        assert not np.array_equal(seen[0], seen[1])


def test_stream_default_noise_is_keyed_by_frame_index():
    """SqairStream without explicit noise: Philox keyed by (the stream's seed, index of the step's first frame)."""
    F = make_flags(k_particles=2, n_steps_per_image=3)
    B, T, seed = 3, 2, (1 << 32) + 5
    K, N, nw = 2, 3, int(F.n_what)
    core = SqairCore(F, HW)
    from sqair_amd.params import init_params
    P = {k: np.asarray(v, np.float32) for k, v in init_params(F, HW, seed=1, jitter=0.05).items()}
    core.set_params(P)
    st = SqairStream(core, B, frames_per_step=T, seed=seed, use_graph=False)
    frames = np.zeros((T, B) + HW, np.float32)
    for i in range(3):
        st.step(frames)
        torch.cuda.synchronize()
        _check(core.noise, S.fill_noise(T, B, K, N, nw, seed=seed, step=i * T))
    st.close()
