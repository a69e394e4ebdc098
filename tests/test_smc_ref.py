"""No GPU: the float64 references the SMC and Philox GPU tests stand on (tests/smc_ref.py), the oracle with a carried state, and
the host-side refusals of sqair_smc_resample_test.

- Philox4x32-10 against the published Random123 known answers.
- The oracle fed in chunks with its state carried equals one whole sequence() exactly, for GRU and LSTM cells; rows gathered from
  particle 0 and given identical noise equal particle 0.
- The reference resampler's invariants (floor / ceil copies, non-decreasing ancestors, zero weights never chosen, ties at u = 0).
- Every refusal of the kernel-level resampler entry point, decided before any HIP call (dummy pointers)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from sqair_amd.data import make_sequences, to_float
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from sqair_amd.params import init_params
from tests import smc_ref as S

HW = (24, 24)


# ---- Philox known answers ------------------------------------------------------------------------------------------------
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    got = S.philox4x32_10(ctr, key)
    assert tuple(int(x) for x in got) == want
    # vectorised: the same answer in every position of a broadcast batch
    many = S.philox4x32_10(tuple(np.full(3, c, np.uint64) for c in ctr), key)
    assert all((m == w).all() for m, w in zip(many, want))


def test_noise_restatement_layout():
    """u entries (the last of every record) are 24-bit values in [0, 1), exactly representable in fp32; eps has standard
    moments; sharding (b0, global_B) and the step select other counters."""
    K, N, nw = 3, 2, 5
    full = S.fill_noise(2, 4, K, N, nw, seed=11, step=3)
    u, eps = full[..., -1], full[..., :-1]
    assert ((u >= 0) & (u < 1)).all() and np.array_equal(u, u.astype(np.float32).astype(np.float64))
    assert np.array_equal(u * 2 ** 24, np.floor(u * 2 ** 24))
    assert abs(eps.mean()) < 0.1 and abs(eps.var() - 1.0) < 0.15
    shard = S.fill_noise(2, 2, K, N, nw, seed=11, step=3, global_B=4, b0=1)
    assert np.array_equal(shard, full[:, K:3 * K])
    assert not np.array_equal(S.fill_noise(2, 4, K, N, nw, seed=11, step=4), full)
    assert not np.array_equal(S.fill_noise(2, 4, K, N, nw, seed=11 + (1 << 32), step=3), full)   # the key's high word counts


# ---- the oracle with a carried state ---------------------------------------------------------------------------------------
def _oracle_case(cells, B=2, K=2, T=5, seed=3):
    flags = dict(k_particles=K, n_steps_per_image=2)
    if cells == "lstm":
        flags.update(time_transition="LSTM", prior_transition="LSTM")
    F = make_flags(**flags)
    obs = to_float(make_sequences(B, T=T, canvas=HW, seed=seed)["imgs"])
    P = {k: np.asarray(v, np.float32) for k, v in init_params(F, HW, seed=seed, mean_img=obs.mean((0, 1)), jitter=0.05).items()}
    orc = O.SqairOracle(P, O.make_cfg(F, HW), torch.float64)
    rng = np.random.default_rng(seed)
    N, nw = int(F.n_steps_per_image), int(F.n_what)
    noise = rng.standard_normal((T, B * K, 2, N, 4 + nw + 1))
    noise[..., -1] = rng.uniform(size=noise.shape[:-1])
    # presence probabilities near 1/2 everywhere would make this test trivially pass on an all-absent run: bias u low
    noise[..., -1] *= 0.6
    tiled = O.tile_input_for_iwae(torch.as_tensor(obs, dtype=torch.float64), K)
    return orc, tiled, torch.as_tensor(noise)


@pytest.mark.parametrize("cells", ["gru", "lstm"])
def test_oracle_chunks_with_carried_state_equal_the_whole_sequence(cells):
    orc, tiled, noise = _oracle_case(cells)
    T = tiled.shape[0]
    with torch.no_grad():
        whole, final = orc.sequence(tiled, noise, return_state=True)
        assert torch.equal(whole["log_weights_per_timestep"], orc.sequence(tiled, noise)["log_weights_per_timestep"])
        assert float(whole["presence"].sum()) > 0 and float(whole["obj_id"].max()) >= 0
        state, parts = None, []
        for t0, t1 in ((0, 2), (2, 3), (3, T)):
            o, state = orc.sequence(tiled[t0:t1], noise[t0:t1], state=state if state is not None else orc.initial_state(tiled.shape[1]),
                                    return_state=True)
            parts.append(o)
    for k in whole:
        if k.startswith("_final"):
            assert torch.equal(parts[-1][k], whole[k]), k
        else:
            assert torch.equal(torch.cat([p[k] for p in parts]), whole[k]), k
    assert torch.equal(state.t, torch.full_like(state.t, T)) and torch.equal(final.t, state.t)
    for x, y in zip((state.temporal, state.prior, state.prev_ids, state.last_id) + state.z,
                    (final.temporal, final.prior, final.prev_ids, final.last_id) + final.z):
        assert torch.equal(x, y)


def test_oracle_step_prior_reads_the_row_counter():
    """The discovery step prior's timestep bias is on where the row's frame counter is > 0: a row gathered fresh (-1) in the
    middle of a stream starts at counter 0 and gives what frame 0 of a new sequence gives."""
    orc, tiled, noise = _oracle_case("gru", T=3)
    R = tiled.shape[1]
    with torch.no_grad():
        _, st = orc.sequence(tiled[:2], noise[:2], return_state=True)
        src = np.arange(R)
        src[0] = -1
        o, st2 = orc.sequence(tiled[2:3], noise[2:3], state=orc.gather_state(st, src), return_state=True)
        fresh = orc.sequence(tiled[2:3], noise[2:3])
    assert int(st2.t[0]) == 1 and (st2.t[1:] == 3).all()
    for k in ("log_weights_per_timestep", "disc_prior_log_prob", "presence", "what"):
        assert torch.equal(o[k][:, 0], fresh[k][:, 0]), k
    assert not torch.equal(o["disc_prior_log_prob"][:, 1], fresh["disc_prior_log_prob"][:, 1])


@pytest.mark.parametrize("cells", ["gru", "lstm"])
def test_oracle_rows_gathered_from_particle_0_equal_particle_0(cells):
    orc, tiled, noise = _oracle_case(cells, B=1, K=3)
    R = tiled.shape[1]
    same = noise.clone()
    same[2:] = noise[2:, :1].expand_as(noise[2:])   # identical noise for every row after the gather
    with torch.no_grad():
        _, st = orc.sequence(tiled[:2], same[:2], return_state=True)
        assert not torch.equal(st.temporal[0], st.temporal[1]) or not torch.equal(st.z[0][0], st.z[0][1])
        o, _ = orc.sequence(tiled[2:], same[2:], state=orc.gather_state(st, np.zeros(R, np.int64)), return_state=True)
    for k, v in o.items():
        v = v if not k.startswith("_final") else v[None]   # (per frame [T, R, ...]; final states [R, ...])
        for r in range(1, R):   # (fp64 matmuls may block rows differently: 1e-12, not bit for bit; decisions exactly)
            assert torch.allclose(v[:, r], v[:, 0], rtol=1e-12, atol=1e-12), (k, r, float((v[:, r] - v[:, 0]).abs().max()))
            if k in ("presence", "obj_id", "prop_pres", "disc_pres"):
                assert torch.equal(v[:, r], v[:, 0]), (k, r)
    if cells == "lstm":   # both halves of the LSTM prior / temporal state travel with the row
        nh = orc.cfg.n_hidden
        g = orc.gather_state(st, np.zeros(R, np.int64))
        assert torch.equal(g.prior[1, :, nh:], st.prior[0, :, nh:]) and torch.equal(g.temporal[2, :, nh:], st.temporal[0, :, nh:])


# ---- the reference resampler -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 7, 64, 65, 256])
def test_reference_resampler_invariants(K):
    rng = np.random.default_rng(K)
    B = 200
    lw = (rng.standard_normal((2, B * K)) * 3).astype(np.float32)
    if K > 1:
        lw[:, ::5] = -np.inf   # zero-weight particles (never a whole lane: K > 1 consecutive rows hold a non-multiple of 5)
    u = rng.uniform(size=B).astype(np.float32)
    u[:3] = [0.0, 1.0 - 2.0 ** -24, 0.5]
    r = S.resample(np.zeros(B * K, np.float32), lw, np.zeros(B), u, K, 1.0)
    live = r.w.e > 0
    assert r.go[np.isfinite(r.ess)].all()
    for b in range(B):
        if not np.isfinite(r.ess[b]):
            continue
        assert 1.0 - 1e-12 <= r.ess[b] <= K * (1 + 1e-12)
        anc = r.anc[b]
        assert (np.diff(anc) >= 0).all() and live[b][anc].all()
        n = np.bincount(anc, minlength=K)
        kw = K * r.w.e[b] / r.w.S[b]
        assert (n >= np.floor(kw - 1e-9)).all() and (n <= np.ceil(kw + 1e-9)).all()
    # equal weights: ESS = K exactly and, at u = 0, the exact ties c_{j-1} = j = threshold give the identity
    eq = S.resample(np.zeros(K, np.float32), np.full((1, K), 2.5, np.float32), np.zeros(1), np.zeros(1, np.float32), K, 1.0)
    assert eq.ess[0] == K and np.array_equal(eq.anc[0], np.arange(K))
    # a non-finite lane never resamples, whatever ess_frac
    bad = np.full((1, K), -np.inf, np.float32)
    nan = np.zeros((1, K), np.float32)
    nan[0, -1] = np.nan
    for x in (bad, nan):
        r = S.resample(np.zeros(K, np.float32), x, np.zeros(1), np.zeros(1, np.float32), K, 1.0)
        assert not r.go[0] and np.array_equal(r.src, np.arange(K)) and np.array_equal(r.log_w, x[0], equal_nan=True)


def test_reference_resampler_never_picks_a_zero_weight_tail():
    """u near 1 puts the last threshold at S: the last particle of POSITIVE weight is chosen, not particle K - 1."""
    K = 8
    e = np.array([1, 2, 0.5, 1, 0, 0, 0, 0], np.float64)
    anc, c, thr = S.systematic(e, np.float64(1.0))
    assert thr[-1] == c[-1] and anc[-1] == 3
    anc, _, _ = S.systematic(e, np.float64(1.0 - 2.0 ** -24))
    assert anc[-1] == 3 and (anc < 4).all() and len(anc) == K


# ---- refusals of sqair_smc_resample_test ----------------------------------------------------------------------------------------
DUMMY = C.c_void_p(0x1000)   # never dereferenced: every call below is refused first


def _smc(**kw):
    f = dict(ess_frac=0.5, seed=7, uniforms=None, log_w=0x3000, log_z=0x3100, log_evidence=0x3200, ess=0x3300, u_out=None,
             resampled=0x3400, src_rows=0x3500)
    f.update(kw)
    return _capi.SqairSmc(**f)


@pytest.mark.parametrize("path", [None, _capi.WIDE_LIB_PATH])
def test_smc_resample_test_refusals(path):
    lib = _capi.lib(path)
    assert "sqair_smc_resample_test" in _capi.EXPORTED_SYMBOLS and lib.sqair_abi_version() == 2
    cfg = make_config(make_flags(k_particles=3, n_steps_per_image=3, n_what=64 if path else 50), (50, 50))
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    try:
        f = lib.sqair_smc_resample_test
        good = _smc()
        assert f(None, DUMMY, 1, 4, 3, DUMMY, C.byref(good), None) == -1
        cases = [
            ((None, 1, 4, 3, DUMMY, C.byref(good)), "null lw"),
            ((DUMMY, 1, 4, 3, DUMMY, None), "null"),
            ((DUMMY, 0, 4, 3, DUMMY, C.byref(good)), "bad T"),
            ((DUMMY, 1, 0, 3, DUMMY, C.byref(good)), "bad T / B / K"),
            ((DUMMY, 1, 4, 0, DUMMY, C.byref(good)), "K <= 256"),
            ((DUMMY, 1, 4, 257, DUMMY, C.byref(good)), "K <= 256"),
            ((DUMMY, 1, 1 << 30, 256, DUMMY, C.byref(good)), "bad T / B / K"),
            ((DUMMY, 1, 4, 3, DUMMY, C.byref(_smc(ess_frac=float("nan")))), "ess_frac"),
            ((DUMMY, 1, 4, 3, DUMMY, C.byref(_smc(ess_frac=1.5))), "ess_frac"),
            ((DUMMY, 1, 4, 3, DUMMY, C.byref(_smc(ess_frac=-0.1))), "ess_frac"),
            ((DUMMY, 1, 4, 3, None, C.byref(_smc())), "t_row without uniforms"),
        ] + [((DUMMY, 1, 4, 3, DUMMY, C.byref(_smc(**{n: None}))), "must not be NULL")
             for n in ("log_w", "log_z", "log_evidence", "ess", "resampled", "src_rows")]
        for args, msg in cases:
            assert f(h, *args, None) == -1, msg
            assert msg.split()[-1] in lib.sqair_last_error(h).decode(), (msg, lib.sqair_last_error(h))
    finally:
        lib.sqair_destroy(h)
