"""-m gpu: SqairStream(resample="systematic") against the fp64 particle filter of tests/smc_ref.py (the oracle with its state
carried, gathered through the device's own ancestors so that both runs stay on one trajectory).

Per step the noise is drawn on the ORACLE filter's presence margin (as hip_util.stable_noise does; the HIP result is never looked
at), then: presence and ids exactly; the per-frame outputs within the live-oracle gate (5e-4 of max(1, |value|)); the per-frame log
weights, the carried ones and log_evidence within 1e-4 relative (the north-star bar; relative to the largest of the value
and the terms summed into it); the decisions and the device's ancestors
against the fp64 resampler run on the ORACLE's weights with the device's uniform, skipping only what the measured log-weight
discrepancy delta allows (|ESS - ess_frac K| within 8 delta ESS; |c_i - thr| <= 2 delta S).  A lane is reset in mid-stream, and
resampling must happen."""
import pytest

from tests.stream_cases import filter_case

pytestmark = pytest.mark.gpu

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


@pytest.mark.parametrize("case", sorted(CASES))
def test_stream_matches_the_fp64_particle_filter(case):
    filter_case(case, *CASES[case])
