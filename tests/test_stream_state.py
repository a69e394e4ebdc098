"""-m gpu: stateful streaming inference (include/sqair_hip.h: sqair_set_state; sqair_amd/stream.py).

A sequence fed in chunks with the state carried from call to call gives the outputs of one pass over the whole sequence, bit for
bit (same frames, same noise slices); lanes can be reset and particles resampled through the source map; one captured graph of a
one-frame pass, replayed with the state updated in place, gives the eager results."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.data import config_inputs
from sqair_amd.stream import SqairStream
from tests.stream_harness import (FINAL, PER_FRAME, blob as _blob, chunked as _chunked, compare, core as _core, one_pass,
                                  set_state, setup, switches)

pytestmark = pytest.mark.gpu

DECODER = ("canvas", "glimpse", "data_ll_per_sample", "log_weights_per_timestep")


def _setup(flags, hw, B, T, seed=11):
    return setup(flags, B, T, hw, seed)


# ---- 1. chunked == whole ---------------------------------------------------------------------------------------------------
CASES = {
    "shipped": (dict(k_particles=2, n_steps_per_image=3), (50, 50), 4, 10),
    "lstm_cells": (dict(k_particles=2, n_steps_per_image=3, time_transition="LSTM", prior_transition="LSTM"), (50, 50), 4, 10),
    "vanilla_cells": (dict(k_particles=2, n_steps_per_image=3, time_transition="VanillaRNN", prior_transition="VanillaRNN"),
                      (50, 50), 4, 10),
    "gru_slot_rnn": (dict(k_particles=2, n_steps_per_image=2, transition="GRU"), (50, 50), 3, 10),
    "rec_where_prior": (dict(k_particles=2, n_steps_per_image=3, rec_where_prior=True, prop_prior_type="guided"), (50, 50), 4, 10),
    "padded_n_units": (dict(k_particles=2, n_steps_per_image=3, n_units=5), (50, 50), 4, 10),
    "frame_37x41": (dict(k_particles=3, n_steps_per_image=3), (37, 41), 5, 10),
    "wide_n_what_64": (dict(k_particles=2, n_steps_per_image=3, n_what=64), (50, 50), 3, 10),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_chunked_passes_equal_the_whole_pass(case):
    flags, hw, B, T = CASES[case]
    F, P, obs, noise = _setup(flags, hw, B, T)
    core = _core(F, hw, P)
    if case.startswith("wide"):
        assert core.lib is _capi.lib(_capi.WIDE_LIB_PATH)
    whole = one_pass(core, obs, noise)
    assert float(whole["presence"].sum()) > 0 and float(whole["obj_id"].max()) >= 0
    R, N = B * int(F.k_particles), int(F.n_steps_per_image)
    for sizes in ([3, 3, 4], [1] * T):
        enc, dec = switches(T, sizes, B, R, N, hw)
        assert not enc and not dec, "the shapes of these cases keep every once-per-pass layer on one kernel"
        got, _ = _chunked(core, obs, noise, sizes)
        compare(got, whole)


@pytest.mark.parametrize("T,sizes,B", [(10, [3, 3, 4], 32), (10, [1] * 10, 32), (100, [10] * 10, 5)],
                         ids=["cfg2_T10_334", "cfg2_T10_ones", "T100_by_10"])
def test_cfg2_chunked_and_long_sequences(T, sizes, B):
    """cfg-2 (K = 5, N = 4) at T = 10: the whole pass's decoder runs on 6400 rows (another kernel than a chunk's); and T = 100 fed
    ten frames at a time (the reference's claim of 100-step sequences), same kernel switch.  Decoder outputs at the gate, the
    rest exact."""
    ov, _, _, _ = config_inputs(2)
    hw = (50, 50)
    F, P, obs, noise = _setup(ov, hw, B, T, seed=5)
    core = _core(F, hw, P)
    whole = one_pass(core, obs, noise)
    R, N = B * int(F.k_particles), int(F.n_steps_per_image)
    enc, dec = switches(T, sizes, B, R, N, hw)
    assert not enc and dec
    got, _ = _chunked(core, obs, noise, sizes)
    compare(got, whole, loose=DECODER)
    assert float(whole["obj_id"][-1].max()) >= 0   # objects carried to the last frame


# ---- 2. one graph, state in place, chain on and off ---------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [0, 1])
def test_graph_replayed_in_place_equals_eager_chunks(chain):
    B, T = 8, 6
    flags, hw = dict(k_particles=2, n_steps_per_image=3), (50, 50)
    F, P, obs, noise = _setup(flags, hw, B, T, seed=21)
    eager, _ = _chunked(_core(F, hw, P, options={"slot_chain": chain}), obs, noise, [1] * T)
    core = _core(F, hw, P, options={"slot_chain": chain})
    R = B * int(F.k_particles)
    core.bind(1, B, "all")
    blob = _blob(core, B)
    src = torch.full((R,), -1, dtype=torch.int32, device=core.device)   # the first replay starts every row fresh
    outs = []
    with core.on_stream():
        set_state(core, B, blob, blob, src)
        core.stream.synchronize()
        core.check(core.lib.sqair_graph_capture(*core._args(0)), "sqair_graph_capture")
        for t in range(T):
            core.obs.copy_(torch.as_tensor(obs[t:t + 1]))
            core.noise.copy_(torch.as_tensor(noise[t:t + 1]).reshape(core.noise.shape))
            core.check(core.lib.sqair_graph_launch(core.handle, core._stream()), "sqair_graph_launch")
            if t == 0:
                src.copy_(torch.arange(R, dtype=torch.int32, device=core.device))
            outs.append({k: v.clone() for k, v in core.out.items()})
    core.stream.synchronize()
    if chain:
        core.check_chain()
    got = {k: np.concatenate([o[k].cpu().numpy() for o in outs]) for k in PER_FRAME}
    got.update({k: outs[-1][k].cpu().numpy() for k in FINAL})
    compare(got, eager)


# ---- 3. reset -------------------------------------------------------------------------------------------------------------------
def test_reset_lane_starts_a_fresh_sequence():
    B, T, j = 4, 6, 2
    flags, hw = dict(k_particles=2, n_steps_per_image=3), (50, 50)
    F, P, obs, noise = _setup(flags, hw, B, T, seed=31)
    K = int(F.k_particles)
    R = B * K
    core = _core(F, hw, P)
    _, cont = _chunked(core, obs, noise, [3, 3])
    src = np.arange(R)
    src[j * K:(j + 1) * K] = -1
    _, reset = _chunked(core, obs, noise, [3, 3], src_before={1: src})
    fresh = one_pass(core, obs[3:], noise[3:])   # same B, t_offset 0, chunk 2's frames
    lane = slice(j * K, (j + 1) * K)
    others = np.r_[0:j * K, (j + 1) * K:R]
    for k in PER_FRAME:
        assert np.array_equal(reset[1][k][:, lane], fresh[k][:, lane], equal_nan=True), k
        assert np.array_equal(reset[1][k][:, others], cont[1][k][:, others], equal_nan=True), k
    for k in FINAL:
        assert np.array_equal(reset[1][k][lane], fresh[k][lane]), k
        assert np.array_equal(reset[1][k][others], cont[1][k][others]), k
    assert not np.array_equal(cont[1]["obj_id"][:, lane], fresh["obj_id"][:, lane]) or \
        not np.array_equal(cont[1]["log_weights_per_timestep"][:, lane], fresh["log_weights_per_timestep"][:, lane])


# ---- 4. resample ----------------------------------------------------------------------------------------------------------------
def test_resample_every_particle_from_particle_zero():
    B, T = 4, 6
    flags, hw = dict(k_particles=3, n_steps_per_image=3), (50, 50)
    F, P, obs, noise = _setup(flags, hw, B, T, seed=41)
    K = int(F.k_particles)
    R = B * K
    noise = noise.copy()
    for b in range(B):   # chunk 2: every particle of a sequence draws particle 0's noise
        noise[3:, b * K:(b + 1) * K] = noise[3:, b * K:b * K + 1]
    core = _core(F, hw, P)
    _, cont = _chunked(core, obs, noise, [3, 3])
    src = np.repeat(np.arange(B) * K, K)       # src[b*K + k] = b*K
    _, res = _chunked(core, obs, noise, [3, 3], src_before={1: src})
    first = np.arange(B) * K
    for k in PER_FRAME:
        for kk in range(K):
            assert np.array_equal(res[1][k][:, first + kk], cont[1][k][:, first], equal_nan=True), (k, kk)
    for k in FINAL:
        for kk in range(K):
            assert np.array_equal(res[1][k][first + kk], cont[1][k][first]), (k, kk)
    # the ids of the resampled particles are those of particle 0: every id seen is at most the row's last used id
    ids, last = res[1]["obj_id"], res[1]["final_last_used_id"]
    assert (ids.max(axis=(0, 2)) <= last).all()
    assert float(res[0]["obj_id"].max()) >= 0
    # without the map the particles differ (the test is not vacuous)
    assert not np.array_equal(cont[1]["log_weights_per_timestep"][:, first + 1], cont[1]["log_weights_per_timestep"][:, first])


# ---- 5. off is off ------------------------------------------------------------------------------------------------------------
def test_graph_nodes_only_the_import_and_export_are_added():
    B = 4
    flags, hw = dict(k_particles=2, n_steps_per_image=3), (50, 50)
    F, P, obs, noise = _setup(flags, hw, B, 2, seed=51)

    def nodes(mode):
        core = _core(F, hw, P)
        core.bind(2, B, "all")
        blob = _blob(core, B)
        with core.on_stream():
            core.obs.copy_(torch.as_tensor(obs))
            core.noise.copy_(torch.as_tensor(noise).reshape(core.noise.shape))
            if mode == "set_then_off":
                set_state(core, B, blob, blob)
                set_state(core, B)
            elif mode == "in_place":
                set_state(core, B, blob, blob)
            elif mode == "export_only":
                set_state(core, B, None, blob)
            core.stream.synchronize()
            core.check(core.lib.sqair_graph_capture(*core._args(0)), "sqair_graph_capture")
        return core.graph_nodes()

    n0 = nodes("never")
    assert n0 > 100
    assert nodes("set_then_off") == n0
    assert nodes("in_place") == n0 + 2
    assert nodes("export_only") == n0 + 2


# ---- 6. SqairStream ------------------------------------------------------------------------------------------------------------
def test_sqair_stream_steps_equal_the_whole_pass():
    B, T = 4, 10
    flags, hw = dict(k_particles=2, n_steps_per_image=3), (50, 50)
    F, P, obs, noise = _setup(flags, hw, B, T, seed=61)
    K = int(F.k_particles)
    R = B * K
    whole = one_pass(_core(F, hw, P), obs, noise)
    core = _core(F, hw, P)
    st = SqairStream(core, B, frames_per_step=1, outputs=PER_FRAME, use_graph=True)
    outs = [st.step(obs[t:t + 1], noise=noise[t:t + 1]) for t in range(T)]
    torch.cuda.synchronize()
    got = {k: np.concatenate([o[k].cpu().numpy() for o in outs]) for k in PER_FRAME}
    for k in PER_FRAME:
        assert np.array_equal(got[k], whole[k], equal_nan=True), k
    assert st.frame == T
    assert np.allclose(st.log_weight_sum.cpu().numpy(), whole["log_weights_per_timestep"].astype(np.float64).sum(0), rtol=1e-5, atol=1e-3)
    # host-side validation
    with pytest.raises(ValueError):
        st.reset([B])
    with pytest.raises(ValueError):
        st.resample(np.arange(R - 1))
    with pytest.raises(ValueError):
        st.resample(np.full(R, R))
    with pytest.raises(ValueError):
        st.step(obs[:2])
    # lane 1 starts the clip again (the same graph replays): its rows equal the whole pass's; a resample that swaps the first two
    # particles of lane 3 moves their log-weight sums with them
    j = 1
    st.reset([j])
    src = np.arange(R)
    src[3 * K], src[3 * K + 1] = 3 * K + 1, 3 * K
    sums = st.log_weight_sum.cpu().numpy().copy()
    st.resample(src)
    outs = [st.step(obs[t:t + 1], noise=noise[t:t + 1]) for t in range(T)]
    torch.cuda.synchronize()
    lane = slice(j * K, (j + 1) * K)
    for k in PER_FRAME:
        g = np.concatenate([o[k].cpu().numpy() for o in outs])
        assert np.array_equal(g[:, lane], whole[k][:, lane], equal_nan=True), k
    lw = np.concatenate([o["log_weights_per_timestep"].cpu().numpy() for o in outs])
    want = sums[src].copy()
    want[lane] = 0.0
    assert np.allclose(st.log_weight_sum.cpu().numpy(), want + lw.astype(np.float64).sum(0), rtol=1e-5, atol=1e-3)
    assert st.frame == 2 * T
    st.close()
    # the handle's plain passes start from the initial state again
    again = one_pass(core, obs, noise)
    for k in PER_FRAME:
        assert np.array_equal(again[k], whole[k], equal_nan=True), k
