"""-m gpu: adjoint kernels (building blocks of the training step) against autograd on the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from tests.hip_util import dev, rel_err, stream

from tests.pass_cases import LOOSE, check_report, full_backward_case

pytestmark = pytest.mark.gpu
D = torch.float64


def _handle(K, N, hw, **flags):
    lib = _capi.lib()
    F = make_flags(k_particles=K, n_steps_per_image=N, **flags)
    cfg = make_config(F, hw)
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h, F


@pytest.mark.parametrize("hw", [(50, 50), (128, 128), (33, 48)])
@pytest.mark.parametrize("masked", [False, True])
def test_st_crop_backward(hw, masked):
    lib, h, F = _handle(3, 4, hw)
    try:
        B, K, G = 4, 3, 20
        R = B * K
        rng = np.random.default_rng(hw[1])
        img = rng.uniform(size=(B,) + hw).astype(np.float32)
        where = (rng.standard_normal((R, 4)) * 1.2).astype(np.float32)
        where[0] = [2.0, 2.5, 0.1, -0.2]
        mask = rng.uniform(size=(R, G * G)).astype(np.float32) if masked else None
        g_out = rng.standard_normal((R, G * G)).astype(np.float32)
        d_where = torch.zeros(R, 4, device="cuda")
        d_mask = torch.zeros(R, G * G, device="cuda")
        di, dw, dg = dev(img), dev(where), dev(g_out)
        dm = dev(mask) if masked else None
        rc = lib.sqair_st_crop_bwd(h, di.data_ptr(), dw.data_ptr(), dm.data_ptr() if masked else None, dg.data_ptr(),
                                   d_where.data_ptr(), d_mask.data_ptr() if masked else None, B, stream())
        assert rc == 0
        torch.cuda.synchronize()
        w64 = torch.tensor(where, dtype=D, requires_grad=True)
        m64 = torch.tensor(mask, dtype=D, requires_grad=True) if masked else None
        out = O.st_crop(torch.tensor(np.repeat(img, K, 0), dtype=D), w64, G).reshape(R, -1)
        if masked:
            out = out * m64
        (out * torch.tensor(g_out, dtype=D)).sum().backward()
        assert rel_err(d_where.cpu().numpy(), w64.grad.numpy()) < 2e-4
        if masked:
            assert rel_err(d_mask.cpu().numpy(), m64.grad.numpy()) < 1e-5
    finally:
        lib.sqair_destroy(h)


@pytest.mark.parametrize("hw,n_slots,G", [((50, 50), 4, 20), ((128, 128), 4, 20), ((77, 130), 4, 20), ((40, 200), 3, 20), ((128, 128), 7, 20),
                                          ((30, 250), 8, 20), ((24, 300), 4, 20), ((90, 65), 1, 20), ((600, 100), 3, 20),
                                          ((128, 128), 4, 5), ((100, 128), 3, 12), ((128, 128), 2, 2)])
def test_st_insert_loglik_backward(hw, n_slots, G):
    # 65 .. 256 columns and up to 8 slots: the row-wave adjoint (k_insert_loglik_bwd_rows); the others the band kernel
    lib, h, F = _handle(2, n_slots, hw, glimpse_size=G)
    try:
        B, K, N = 3, 2, n_slots
        R = B * K
        H, W = hw
        rng = np.random.default_rng(5)
        gl = (rng.standard_normal((R, N, G * G)) * 0.3).astype(np.float32)
        where = rng.standard_normal((R, N, 4)).astype(np.float32)
        pres = (rng.uniform(size=(R, N)) > 0.35).astype(np.float32)
        pres[1] = 0.0
        img = rng.uniform(size=(B, H, W)).astype(np.float32)
        mean_img = rng.uniform(size=(H, W)).astype(np.float32)
        g_ll = rng.standard_normal(R).astype(np.float32)
        d_gl = torch.zeros(R, N, G * G, device="cuda")
        d_wh = torch.zeros(R, N, 4, device="cuda")
        d_mean = torch.zeros(H, W, device="cuda")
        scratch = torch.empty(R * H * W, device="cuda")
        ts = [dev(gl), dev(where), dev(pres), dev(img), dev(mean_img), dev(g_ll)]
        rc = lib.sqair_st_insert_loglik_bwd(h, *[t.data_ptr() for t in ts], d_gl.data_ptr(), d_wh.data_ptr(),
                                            d_mean.data_ptr(), scratch.data_ptr(), scratch.numel() * 4, B, stream())
        assert rc == 0
        torch.cuda.synchronize()
        ocfg = O.make_cfg(F, hw)
        g64 = torch.tensor(gl, dtype=D, requires_grad=True)
        w64 = torch.tensor(where, dtype=D, requires_grad=True)
        mi64 = torch.tensor(mean_img, dtype=D, requires_grad=True)
        p64 = torch.tensor(pres, dtype=D)
        gg = g64.reshape(R * N, G, G)
        ww = w64.reshape(R * N, 4)
        inv = O.st_insert(gg, ww, H, W).reshape(R, N, H, W) * p64[..., None, None]
        nz = (O.st_insert(torch.ones_like(gg), ww, H, W).reshape(R, N, H, W) * p64[..., None, None]).sum(1)
        nz = torch.sigmoid(-10.0 + 20.0 * nz)
        cv = inv.sum(1) + mi64[None] * nz
        std = nz * ocfg.output_std + (1 - nz) * ocfg.background_std
        ll = O.normal_log_prob(torch.tensor(np.repeat(img, K, 0), dtype=D), cv, std).sum((1, 2))
        (ll * torch.tensor(g_ll, dtype=D)).sum().backward()
        assert rel_err(d_gl.cpu().numpy(), g64.grad.numpy()) < 1e-4
        assert rel_err(d_mean.cpu().numpy(), mi64.grad.numpy()) < 1e-4
        assert rel_err(d_wh.cpu().numpy(), w64.grad.numpy()) < 5e-4
    finally:
        lib.sqair_destroy(h)


@pytest.mark.parametrize("B,K,T", [(32, 5, 10), (5, 3, 4)])
def test_elbo_backward(B, K, T):
    lib, h, F = _handle(K, 3, (50, 50))
    try:
        rng = np.random.default_rng(B)
        lw_t = (rng.standard_normal((T, B * K)) * 20.0 + 300.0).astype(np.float32)
        dl_t = (rng.standard_normal((T, B * K)) * 2.0 - 3.0).astype(np.float32)
        d_lw, d_dl = dev(lw_t), dev(dl_t)
        lw = torch.zeros(B, K, device="cuda"); el = torch.zeros(B, device="cuda"); iw = torch.zeros(B, K, device="cuda")
        sig = torch.zeros(B, K, device="cuda"); sc = torch.zeros(16, device="cuda"); mo = torch.zeros(8, device="cuda")
        means = (C.c_void_p * 8)(*([None] * 8))
        assert lib.sqair_elbo(h, d_lw.data_ptr(), d_dl.data_ptr(), T, B, lw.data_ptr(), el.data_ptr(), iw.data_ptr(),
                              sig.data_ptr(), sc.data_ptr(), means, 0, mo.data_ptr(), stream()) == 0
        g_lw = torch.zeros(T, B * K, device="cuda"); g_dl = torch.zeros(T, B * K, device="cuda")
        assert lib.sqair_elbo_bwd(h, iw.data_ptr(), sig.data_ptr(), T, B, g_lw.data_ptr(), g_dl.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        a = torch.tensor(lw_t, dtype=D, requires_grad=True)
        b = torch.tensor(dl_t, dtype=D, requires_grad=True)
        LW = a.sum(0).reshape(B, K)
        tgt = O.vimco(LW, b.sum(0).reshape(B, K), O.iwae(LW)) / T
        tgt.backward()
        assert np.abs(g_lw.cpu().numpy() - a.grad.numpy()).max() < 5e-3 * np.abs(a.grad.numpy()).max()
        assert np.abs(g_dl.cpu().numpy() - b.grad.numpy()).max() < 5e-3 * np.abs(b.grad.numpy()).max()
    finally:
        lib.sqair_destroy(h)


@pytest.mark.parametrize("K", [5, 70])
def test_elbo_reinforce_signal(K):
    """sqair_set_option("vi_target", 1): the plain REINFORCE target of sqair/targets.py:78-89 (stop_gradient(log w) as the learning
    signal, no control variate) -- signal, proxy loss and the gradients of both inputs against the oracle's restatement."""
    B, T = 6, 4
    lib, h, F = _handle(K, 3, (50, 50))
    try:
        assert lib.sqair_set_option(h, b"vi_target", 1) == 0
        rng = np.random.default_rng(K)
        lw_t = (rng.standard_normal((T, B * K)) * 20.0 + 300.0).astype(np.float32)
        dl_t = (rng.standard_normal((T, B * K)) * 2.0 - 3.0).astype(np.float32)
        d_lw, d_dl = dev(lw_t), dev(dl_t)
        lw = torch.zeros(B, K, device="cuda"); el = torch.zeros(B, device="cuda"); iw = torch.zeros(B, K, device="cuda")
        sig = torch.zeros(B, K, device="cuda"); sc = torch.zeros(16, device="cuda"); mo = torch.zeros(8, device="cuda")
        means = (C.c_void_p * 8)(*([None] * 8))
        assert lib.sqair_elbo(h, d_lw.data_ptr(), d_dl.data_ptr(), T, B, lw.data_ptr(), el.data_ptr(), iw.data_ptr(),
                              sig.data_ptr(), sc.data_ptr(), means, 0, mo.data_ptr(), stream()) == 0
        g_lw = torch.zeros(T, B * K, device="cuda"); g_dl = torch.zeros(T, B * K, device="cuda")
        assert lib.sqair_elbo_bwd(h, iw.data_ptr(), sig.data_ptr(), T, B, g_lw.data_ptr(), g_dl.data_ptr(), stream()) == 0
        torch.cuda.synchronize()
        a = torch.tensor(lw_t, dtype=D, requires_grad=True)
        b = torch.tensor(dl_t, dtype=D, requires_grad=True)
        LW = a.sum(0).reshape(B, K)
        tgt = O.reinforce(LW, b.sum(0).reshape(B, K), O.iwae(LW)) / T
        tgt.backward()
        assert np.array_equal(sig.cpu().numpy(), lw_t.sum(0, dtype=np.float32).reshape(B, K)) or \
            rel_err(sig.cpu().numpy(), LW.detach().numpy()) < 1e-6
        assert abs(float(sc[2]) - float(tgt.detach())) <= 1e-5 * abs(float(tgt.detach()))
        assert np.abs(g_lw.cpu().numpy() - a.grad.numpy()).max() < 5e-3 * np.abs(a.grad.numpy()).max()
        assert np.abs(g_dl.cpu().numpy() - b.grad.numpy()).max() < 5e-3 * np.abs(b.grad.numpy()).max()
        assert lib.sqair_set_option(h, b"vi_target", 2) != 0   # only 0 / 1
    finally:
        lib.sqair_destroy(h)


def _wgrad_launches(lib):
    """(blocks flushed through k_wgrad_group, own launches of sq_launch_wgrad_acc) by this process so far."""
    grouped, own = C.c_int64(-1), C.c_int64(-1)
    assert lib.sqair_debug_wgrad_launches(C.byref(grouped), C.byref(own)) == 0
    return grouped.value, own.value


@pytest.mark.parametrize("M,K,N,act", [(160, 256, 256, 1), (640, 400, 256, 1), (6400, 56, 256, 1), (160, 311, 128, 2),
                                       (37, 54, 109, 0), (160, 256, 100, 4), (33, 128, 400, 3), (37, 56, 112, 1),
                                       (160, 576, 256, 1)])
def test_linear_backward_mfma(M, K, N, act):
    """One dense layer backward on the kernels the training step runs: dx through k_linear on the transposed pack, dw / db routed as
    sqair_backward routes a block.  K % 4 != 0 (311, 54: x's rows are not 16-byte aligned) goes to k_wgrad2 as its own launch,
    every other shape to k_wgrad_group: 6400 rows are five M-chunks that meet through atomics, 37 rows a partial 16-row step,
    K = 56 less than one 64-wide tile, 576 x 256 = 36 tiles dealt in two groups."""
    lib, h, F = _handle(2, 3, (50, 50))
    try:
        before = _wgrad_launches(lib)
        rng = np.random.default_rng(M + K)
        x = rng.standard_normal((M, K)).astype(np.float32)
        w = (rng.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
        b = (rng.standard_normal(N) * 0.1).astype(np.float32)
        dy = rng.standard_normal((M, N)).astype(np.float32)
        fn = [lambda v: v, O.elu, torch.tanh, torch.sigmoid, lambda v: O.softplus(v) + 1e-2][act]
        x64 = torch.tensor(x, dtype=D, requires_grad=True)
        w64 = torch.tensor(w, dtype=D, requires_grad=True)
        b64 = torch.tensor(b, dtype=D, requires_grad=True)
        y64 = fn(x64 @ w64 + b64)
        (y64 * torch.tensor(dy, dtype=D)).sum().backward()
        dxx, dww, dyy, dy_out = dev(x), dev(w), dev(dy), dev(y64.detach().numpy())
        dx = torch.zeros(M, K, device="cuda"); dw = torch.zeros(K, N, device="cuda"); db = torch.zeros(N, device="cuda")
        nel = ((N + 15) // 16) * ((K + 15) // 16) * 256
        scratch = torch.empty(2 * nel + 4096 + M * (N + 4) * 2, dtype=torch.float32, device="cuda")
        rc = lib.sqair_linear_bwd_test(h, dxx.data_ptr(), dww.data_ptr(), dy_out.data_ptr(), dyy.data_ptr(), dx.data_ptr(),
                                       dw.data_ptr(), db.data_ptr(), M, K, N, act, scratch.data_ptr(), scratch.numel() * 4,
                                       stream())
        assert rc == 0, lib.sqair_last_error(h)
        grouped, own = (a - b for a, b in zip(_wgrad_launches(lib), before))
        assert (grouped, own) == ((0, 1) if K % 4 else (1, 0))
        assert rel_err(dx.cpu().numpy(), x64.grad.numpy()) < 2e-5
        assert rel_err(dw.cpu().numpy(), w64.grad.numpy()) < 2e-5 * max(1.0, np.sqrt(M / 160.0))
        assert rel_err(db.cpu().numpy(), b64.grad.numpy()) < 2e-5 * max(1.0, np.sqrt(M / 160.0))
    finally:
        lib.sqair_destroy(h)


@pytest.mark.parametrize("K,N,T,B,hw", [(5, 4, 5, 3, (50, 50)), (2, 3, 3, 4, (32, 40))])
def test_backward_decoder_branch_matches_autograd(K, N, T, B, hw):
    """Gradients of the VIMCO target w.r.t. every decoder parameter (they depend on the decoder path only) after a
    full HIP forward pass, against autograd through the whole oracle model."""
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.model import Model, SqairCore
    from tests.hip_util import draw_noise, params32
    F = make_flags(k_particles=K, n_steps_per_image=N)
    d = make_sequences(B, T=T, canvas=hw, n_objects=(1, 2), obj_size=min(28, hw[0] // 2), seed=11)
    obs = to_float(d["imgs"])
    P = params32(F, hw, 4, 0.05, obs.mean((0, 1)))
    core = SqairCore(F, hw)
    core.set_params(P)
    names = ["log_weights_per_timestep", "discrete_log_prob", "presence", "prop_pres", "disc_pres"]
    m = Model(obs, None, core, K, outputs=names)
    from tests.hip_util import stable_noise
    noise, ref, orc, _ = stable_noise(F, hw, P, obs, T, B * K, N, seed0=100, requires_grad=True)
    m.run(noise=noise)
    torch.cuda.synchronize()
    assert np.array_equal(m.prop_pres.cpu().numpy(), ref.prop_pres.detach().numpy())
    assert np.array_equal(m.disc_pres.cpu().numpy(), ref.disc_pres.detach().numpy())
    orc.make_target(ref).backward()
    # the caller's gradient buffer arrives full of a sentinel: the entry overwrites the eight dec.* ranges and nothing else
    flat_grad = torch.full_like(core.flat, 7.25)
    grads, d_rec = core.backward_decoder(flat_grad=flat_grad)
    assert sorted(grads) == ["dec.l0.b", "dec.l0.w", "dec.l1.b", "dec.l1.w", "dec.l2.b", "dec.l2.w", "dec.mean_img", "dec.output_scale"]
    other = torch.ones(flat_grad.numel(), dtype=torch.bool)
    for name, (o, shape) in core.offsets.items():
        if name.startswith("dec."):
            other[o:o + (int(np.prod(shape)) if len(shape) else 1)] = False
    assert other.sum() > 0 and bool((flat_grad.cpu()[other] == 7.25).all())
    for name, g in grads.items():
        want = orc.P[name].grad.numpy()
        got = g.cpu().numpy().reshape(want.shape)
        assert np.abs(got - want).max() <= 2e-3 * max(np.abs(want).max(), 1e-12), (name, np.abs(got - want).max(), np.abs(want).max())
    assert np.isfinite(d_rec.cpu().numpy()).all() and float(d_rec.abs().sum()) > 0


def test_rmsprop_step_matches_tf_semantics():
    from sqair_amd.train import rmsprop_reference
    lib, h, F = _handle(2, 3, (50, 50))
    try:
        n = 2951522 + 3  # not a multiple of 4: exercises the scalar tail
        rng = np.random.default_rng(0)
        theta = rng.standard_normal(n).astype(np.float32)
        ms = np.ones(n, dtype=np.float32)
        mom = np.zeros(n, dtype=np.float32)
        dt, dms, dmom = dev(theta), dev(ms), dev(mom)
        t64, s64, m64 = theta.astype(np.float64), ms.astype(np.float64), mom.astype(np.float64)
        for it in range(3):
            g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1)).astype(np.float32)
            dg = dev(g * 2.0)  # as if summed over 2 ranks; grad_scale = 0.5 undoes it
            assert lib.sqair_rmsprop_step(h, dt.data_ptr(), dg.data_ptr(), dms.data_ptr(), dmom.data_ptr(), n, 1e-3, 0.9, 0.9,
                                          1e-10, 0.5, stream()) == 0
            t64, s64, m64 = rmsprop_reference(t64, g.astype(np.float64), s64, m64, 1e-3)
        torch.cuda.synchronize()
        assert np.abs(dt.cpu().numpy() - t64).max() < 1e-5
        assert rel_err(dms.cpu().numpy(), s64) < 1e-5
    finally:
        lib.sqair_destroy(h)


def test_full_backward_single_frame_discovery_only():
    """T = 1: only discovery, the decoder and the priors are active (propagation sees no present object)."""
    report, _, _ = full_backward_case(K=3, N=3, T=1, B=3, hw=(50, 50), seed=5)
    check_report(report)


@pytest.mark.parametrize("K,N,T,B", [(2, 1, 2, 1), (2, 2, 2, 9), (3, 1, 3, 6)])
def test_full_backward_degenerate_sizes(K, N, T, B):
    """One slot, one sequence, and row counts that leave a last 16-row tile of 2 rows (18 rows): every parameter's gradient
    against autograd through the fp64 oracle."""
    report, _, _ = full_backward_case(K, N, T, B, (50, 50), seed=7)
    check_report(report)


@pytest.mark.parametrize("K,N,T,B,hw", [(3, 3, 3, 3, (50, 50)), (5, 4, 4, 2, (50, 50))])
def test_full_backward_matches_autograd(K, N, T, B, hw):
    """Gradient of the VIMCO target w.r.t. EVERY parameter through the whole recurrence (propagation + discovery +
    compaction + decoder) against autograd through the fp64 oracle, same noise and identical presence decisions.

    What "compaction" means here: at the initialisation's prop_step_bias = 5 a propagated object survives with p ~ 0.993, and these
    two cases (27 and 40 (frame, row) cells) never drop one -- no cell with a survivor behind a dropped slot, 9 and 15 cells where
    prop + disc > N.  They cover the compaction adjoint as the identity on the propagated slots plus truncation of the discoveries.
    Real permutations (holes, holes with discoveries, rows that lose everything), forward and backward, are required and tested in
    tests/test_presence_paths.py; every presence pattern of the kernels themselves in tests/test_compact_kernel.py."""
    report, ref, _ = full_backward_case(K, N, T, B, hw, seed=11)
    assert float(ref.prop_pres.detach().sum()) > 0, "case must exercise propagation"
    check_report(report)


@pytest.mark.parametrize("cell", ["GRU", "LSTM"])
def test_grad_step_graph_replay_equals_eager(cell):
    """forward(train) + ELBO + backward replayed as one HIP graph gives the eager gradients (float atomics in the
    small-parameter adjoints make the order of additions free: compare to 1e-5 of the largest gradient)."""
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.model import Model, SqairCore
    from tests.hip_util import draw_noise, params32
    K, N, T, B, hw = 3, 3, 3, 4, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N, time_transition=cell)
    obs = to_float(make_sequences(B, T=T, canvas=hw, seed=3)["imgs"])
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 4, 0.05, obs.mean((0, 1))))
    Model(obs, None, core, K, outputs="minimal")
    core.noise.copy_(torch.as_tensor(draw_noise(np.random.default_rng(0), T, B * K, N, 55)).reshape(core.noise.shape))
    g0 = core.grad_step(use_graph=False).clone()
    torch.cuda.synchronize()
    for _ in range(2):
        g1 = core.grad_step(use_graph=True).clone()
        torch.cuda.synchronize()
        assert core.train_graph_nodes > 100
        assert float((g1 - g0).abs().max()) <= 1e-5 * float(g0.abs().max())
    # new noise through the same graph changes the result (the graph reads the buffers, not a snapshot)
    core.noise.copy_(torch.as_tensor(draw_noise(np.random.default_rng(1), T, B * K, N, 55)).reshape(core.noise.shape))
    g2 = core.grad_step(use_graph=True).clone()
    torch.cuda.synchronize()
    assert float((g2 - g0).abs().max()) > 1e-3 * float(g0.abs().max())


@pytest.mark.parametrize("cells", [{}, dict(transition="LSTM", time_transition="LSTM", prior_transition="LSTM")])
def test_training_steps_track_oracle_rmsprop(cells):
    """Three optimiser steps (graph replay + fused RMSProp + re-pack) against autograd + the NumPy restatement of the TF
    update on the fp64 oracle, same noise per step.  Every step starts from the HIP path's own fp32 parameters (the
    objective is curved enough that an fp32 rounding of the parameters changes the next gradient by ~1 %), while the
    optimiser slots (ms, mom) are carried independently on both sides."""
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.model import Model, SqairCore
    from sqair_amd.params import flatten_params, unflatten_params
    from sqair_amd.train import Trainer, learning_rate, rmsprop_reference
    from tests.hip_util import draw_noise, params32
    K, N, T, B, hw = 3, 3, 3, 3, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N, learning_rate=1e-3, train_itr=100, **cells)
    obs = to_float(make_sequences(B, T=T, canvas=hw, n_objects=(1, 2), obj_size=24, seed=11)["imgs"])
    P = params32(F, hw, 4, 0.05, obs.mean((0, 1)))
    core = SqairCore(F, hw)
    core.set_params(P)
    m = Model(obs, None, core, K, outputs=["log_weights_per_timestep", "discrete_log_prob", "prop_pres", "disc_pres"])
    tr = Trainer(m, F)
    ms = mom = None
    for it in range(3):
        theta = core.flat.cpu().numpy().astype(np.float64)
        if ms is None:
            ms, mom = np.ones_like(theta), np.zeros_like(theta)
        from tests.hip_util import stable_noise
        noise, ref, orc, _ = stable_noise(F, hw, unflatten_params(theta.astype(np.float32), core.spec), obs, T, B * K, N,
                                          seed0=200 + 10 * it, requires_grad=True)
        target = orc.make_target(ref)
        target.backward()
        tr.step(noise=noise)
        torch.cuda.synchronize()
        # the draw was chosen on the oracle's decision margin: a divergence here is a failure, not a skip
        assert np.array_equal(core.out["prop_pres"].cpu().numpy(), ref.prop_pres.detach().numpy()), it
        assert np.array_equal(core.out["disc_pres"].cpu().numpy(), ref.disc_pres.detach().numpy()), it
        assert abs(float(core.scalars[2]) - float(target)) <= 1e-4 * abs(float(target))
        g = flatten_params({k: (v.grad.numpy() if v.grad is not None else np.zeros(v.shape)) for k, v in orc.P.items()},
                           core.spec).astype(np.float64)
        new, ms, mom = rmsprop_reference(theta, g, ms, mom, learning_rate(F, it))
        got = core.flat.cpu().numpy().astype(np.float64)
        assert np.abs(new - theta).max() > 1e-4
        assert np.abs((got - theta) - (new - theta)).max() <= 2e-3 * np.abs(new - theta).max(), it
    assert tr.step_no == 3


@pytest.mark.parametrize("kind", ["sgd", "momentum", "adam"])
def test_other_optimisers_move_parameters(kind):
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.model import Model, SqairCore
    from sqair_amd.train import Trainer
    from tests.hip_util import params32
    K, N, T, B, hw = 2, 3, 2, 2, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N, learning_rate=1e-4, opt=kind, l2=1e-3)
    obs = to_float(make_sequences(B, T=T, canvas=hw, seed=2)["imgs"])
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 4, 0.05, obs.mean((0, 1))))
    m = Model(obs, None, core, K, outputs="minimal")
    before = core.flat.clone()
    tr = Trainer(m, F)
    tr.step(generator=torch.Generator(device="cuda").manual_seed(0))
    tr.step(generator=torch.Generator(device="cuda").manual_seed(1))
    torch.cuda.synchronize()
    assert torch.isfinite(core.flat).all()
    assert float((core.flat - before).abs().max()) > 0


def test_full_size_cfg2_backward_is_finite_and_times():
    """BASELINE configs[1] shape (T10, 50x50, B32, K5, N4): a whole gradient evaluation as one graph replay."""
    import time
    from sqair_amd.data import config_inputs
    from sqair_amd.model import Model, SqairCore
    from tests.hip_util import params32
    ov, obs, _, _ = config_inputs(2)
    F = make_flags(**ov)
    hw = obs.shape[2:4]
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 1, 0.02, obs.mean((0, 1))))
    Model(obs, None, core, int(F.k_particles), outputs="minimal")
    core.draw_noise(torch.Generator(device="cuda").manual_seed(0))
    g = core.grad_step(use_graph=True)
    torch.cuda.synchronize()
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    t0 = time.perf_counter()
    for _ in range(5):
        core.grad_step(use_graph=True)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 5
    print("cfg2 gradient evaluation: %.2f ms (%d graph nodes)" % (dt * 1e3, core.train_graph_nodes))


def test_checkpoint_round_trip_restores_parameters_and_optimiser_slots(tmp_path):
    """a checkpoint keyed by TF variable names restores parameters, RMSProp slots and the step."""
    from sqair_amd import checkpoint as ck
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.model import Model, SqairCore
    from sqair_amd.train import Trainer
    from tests.hip_util import params32
    K, N, T, B, hw = 2, 3, 2, 2, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N, learning_rate=1e-4)
    obs = to_float(make_sequences(B, T=T, canvas=hw, seed=2)["imgs"])
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 4, 0.05, obs.mean((0, 1))))
    tr = Trainer(Model(obs, None, core, K, outputs="minimal"), F)
    for i in range(2):
        tr.step(generator=torch.Generator(device="cuda").manual_seed(i))
    torch.cuda.synchronize()
    path = str(tmp_path / "model.ckpt.npz")
    ck.save_checkpoint(path, core, tr.opt, global_step=tr.step_no)
    core2 = SqairCore(F, hw)
    core2.set_params(params32(F, hw, 9, 0.05))
    tr2 = Trainer(Model(obs, None, core2, K, outputs="minimal"), F)
    step = ck.load_checkpoint(path, core2, tr2.opt)
    torch.cuda.synchronize()
    assert step == 2
    assert torch.equal(core2.flat, core.flat) and torch.equal(tr2.opt.ms, tr.opt.ms) and torch.equal(tr2.opt.mom, tr.opt.mom)
    # and the restored model evaluates identically
    g = torch.Generator(device="cuda")
    for c in (core, core2):
        with c.on_stream():
            c.draw_noise(g.manual_seed(5))
            c.forward()
        c.stream.synchronize()
    assert torch.equal(core.log_weights, core2.log_weights)


@pytest.mark.parametrize("flags", [
    dict(prop_prior_type="rw"),
    dict(prop_prior_type="guided", masked_glimpse=False),
    dict(disc_prior_type="geom", rec_where_prior=False),
    dict(time_transition="LSTM"),
    dict(prior_transition="LSTM"),
    dict(time_transition="LSTM", prior_transition="LSTM", prop_prior_type="guided"),
    dict(transition="LSTM"),
    dict(transition="GRU"),
    dict(time_transition="VanillaRNN", prior_transition="VanillaRNN"),
    dict(transition="GRU", time_transition="VanillaRNN", prior_transition="LSTM"),
    dict(transition="LSTM", time_transition="LSTM", prior_transition="LSTM"),
])
def test_full_backward_flag_variants(flags):
    """The adjoint branches the default flags never take: random-walk / guided propagation priors (the prior statistics
    feed back into z_{t-1}), geometric step prior, fixed where prior, unmasked glimpses, the LSTM temporal / prior / slot-RNN cells."""
    report, ref, _ = full_backward_case(K=3, N=3, T=3, B=3, hw=(50, 50), seed=11, flags=flags)
    assert float(ref.prop_pres.detach().sum()) > 0
    check_report(report)


@pytest.mark.parametrize("flags", [dict(), dict(prop_prior_type="guided", masked_glimpse=False), dict(transition="LSTM", time_transition="LSTM"),
                                   dict(disc_prior_type="geom", rec_where_prior=False)])
def test_scratch_the_backward_pass_does_not_clear_is_written_in_full(flags, monkeypatch):
    """`sqair_backward` clears only part of its scratch (carve_bwd, sqair_train.hip): the rest it claims to write in full before
    reading it.  The knob build of the library fills that rest with NaNs ahead of the pass (SQAIR_SCRATCH_POISON); every
    gradient must come out as on the product library."""
    knob_lib = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bin", "libsqair_hip_knobs.so")
    if not os.path.exists(knob_lib):
        pytest.skip("knob build of the library not present (python sqair_amd/csrc/build.py --knobs)")
    monkeypatch.setenv("SQAIR_SCRATCH_POISON", "1")
    report, _, _ = full_backward_case(K=3, N=3, T=3, B=3, hw=(50, 50), seed=11, flags=flags, lib_path=knob_lib)
    check_report(report)
    report, _, _ = full_backward_case(K=2, N=3, T=1, B=2, hw=(50, 50), seed=5, flags=flags, lib_path=knob_lib)
    check_report(report)


@pytest.mark.parametrize("flags", [dict(n_units=4), dict(n_what=20), dict(n_what=7), dict(glimpse_size=12), dict(glimpse_size=28),
                                   dict(n_units=4, n_what=7, glimpse_size=12), dict(n_units=2), dict(n_units=3), dict(n_units=6),
                                   dict(n_units=7, transition="LSTM", time_transition="LSTM", prior_transition="LSTM"),
                                   dict(n_units=2, transition="GRU")])
def test_model_size_flags_forward_and_backward(flags):
    """n_units (n_hidden = 32 * n_units; the reference's own --test_run uses n_units = 4, scripts/experiment.py:95), n_what and
    glimpse_size other than the shipped 8 / 50 / 20: all outputs feeding the objective and every gradient against the oracle.
    n_hidden values that are not a multiple of 128 run on layers padded with inert units (csrc/sqair_internal.h: SqairHandle); the
    parameters, their gradients and the final recurrent states cross the ABI in the reference's own shapes."""
    report, ref, core = full_backward_case(K=3, N=3, T=3, B=3, hw=(50, 50), seed=11, flags=flags)
    assert float(ref.prop_pres.detach().sum()) > 0
    lw = core.out["log_weights_per_timestep"].cpu().numpy()
    want = ref.log_weights_per_timestep.detach().numpy()
    assert np.abs(lw - want).max() <= 1e-4 * np.abs(want).max()
    check_report(report)


@pytest.mark.parametrize("K,N,flags", [(3, 3, dict(n_what=64)), (3, 3, dict(n_what=100)), (2, 3, dict(n_what=128, glimpse_size=12)),
                                       (3, 3, dict(n_units=12)), (2, 3, dict(n_units=16)), (2, 12, {}), (2, 9, dict(n_units=2)),
                                       (2, 3, dict(n_units=10, n_what=70, transition="LSTM", time_transition="LSTM", prior_transition="LSTM")),
                                       (2, 3, dict(n_what=60, transition="GRU", prop_prior_type="guided", disc_prior_type="geom"))])
def test_wide_flag_range_forward_and_backward(K, N, flags):
    """The rest of the reference's flag range (n_what > 50, more than 8 object slots, n_units > 8:
    sqair/common_model_flags.py:32-56 and configs/mlp_mnist_model.py:42-52 accept any value) runs on libsqair_hip_wide.so -- the
    same sources with a larger slot record and plain-loop per-row kernels, picked by SqairCore from the flags: the log-weights and
    every gradient against the oracle, exactly like the shipped sizes."""
    from sqair_amd import _capi
    report, ref, core = full_backward_case(K=K, N=N, T=3 if N < 9 else 2, B=2, hw=(50, 50), seed=11, flags=flags)
    assert core.lib is _capi.lib(_capi.WIDE_LIB_PATH)
    assert float(ref.prop_pres.detach().sum()) > 0
    lw = core.out["log_weights_per_timestep"].cpu().numpy()
    want = ref.log_weights_per_timestep.detach().numpy()
    assert np.abs(lw - want).max() <= 1e-4 * np.abs(want).max()
    check_report(report, ill_scale=True)


def test_scalar_hyper_parameter_flags_reach_the_kernels():
    """output_std, scale_prior, prop_prior_step_bias, step_success_prob away from their defaults (with the priors that
    read them: geometric step prior, fixed where prior): objective and gradients against the oracle."""
    flags = dict(output_std=0.2, scale_prior="-1.5", prop_prior_step_bias=4.0, step_success_prob=0.6, disc_prior_type="geom",
                 rec_where_prior=False, transform_var_bias=-2.0, output_scale=0.3, disc_step_bias=0.5, prop_step_bias=3.0)
    report, ref, core = full_backward_case(K=3, N=3, T=3, B=3, hw=(50, 50), seed=11, flags=flags)
    lw = core.out["log_weights_per_timestep"].cpu().numpy()
    want = ref.log_weights_per_timestep.detach().numpy()
    assert np.abs(lw - want).max() <= 1e-4 * np.abs(want).max()
    check_report(report)


@pytest.mark.parametrize("K,N,T,B,hw", [(2, 6, 2, 2, (50, 50)), (2, 3, 2, 2, (128, 128)), (4, 2, 3, 5, (40, 56)), (3, 3, 2, 3, (37, 44)),
                                        (2, 3, 2, 3, (51, 49)), (2, 2, 2, 2, (37, 41)), (128, 2, 2, 1, (50, 50)), (70, 3, 2, 2, (40, 40)),
                                        (2, 5, 2, 2, (96, 128)), (2, 4, 2, 2, (70, 150))])
def test_full_backward_other_shapes(K, N, T, B, hw):
    """N = 6 slots (BASELINE configs[3]), 128x128 frames (configs[4]: the frame no longer fits the default LDS window; the decoder
    canvas and its adjoint run on the row-wave kernels), a non-square frame with B*K not a multiple of the 16-row MFMA tile, frames
    whose H * W is not a multiple of 4 (they pass through a zero-padded copy), more particles than a wavefront has lanes (K = 70, 128:
    the generic ELBO kernel), 5 slots on 96 x 128 (row-wave forward with 8 slot registers, band adjoint), 70 x 150 (four columns per
    lane forward, band adjoint)."""
    report, _, _ = full_backward_case(K, N, T, B, hw, seed=21)
    check_report(report)


@pytest.mark.parametrize("hw", [(12, 14), (3, 250), (257, 5), (150, 256)])
def test_full_backward_extreme_frame_shapes(hw):
    """Frames smaller than the glimpse, degenerate aspect ratios, and the largest frame training takes (38 400 pixels: the crop
    adjoint stages the frame in LDS): every parameter's gradient against autograd through the fp64 oracle."""
    report, _, _ = full_backward_case(2, 2, 2, 2, hw, seed=21)
    check_report(report)


def test_one_particle_trains_with_reinforce_and_vimco_says_why_not():
    """k_particles = 1: VIMCO's leave-one-out baseline divides by K - 1 (targets.py:55; NaN in the reference) -- make_target says so;
    the REINFORCE signal is defined, and its gradient matches autograd through the oracle's reinforce()."""
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.model import Model, SqairCore
    from sqair_amd.train import Optimizer
    from tests.hip_util import params32
    hw, T, B, K, N = (50, 50), 2, 3, 1, 2
    F = make_flags(k_particles=K, n_steps_per_image=N)
    d = make_sequences(B, T=T, canvas=hw, seed=1)
    obs = to_float(d["imgs"])
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 0, 0.05, obs.mean((0, 1))))
    m = Model(obs, None, core, K, presence=d["nums"])
    with pytest.raises(ValueError, match="k_particles >= 2"):
        m.make_target(Optimizer(core))
    target, gvs = m.make_target(Optimizer(core), vi_target="reinforce")
    assert np.isfinite(float(target)) and bool(torch.isfinite(core.flat_grad).all())
    assert abs(float(m.elbo_iwae) - float(m.elbo_vae)) <= 1e-5 * abs(float(m.elbo_vae))   # one particle: the two bounds coincide


def test_training_refuses_frames_it_cannot_stage():
    """One pixel row beyond 38 400 pixels: inference runs, the training entry points say why they do not."""
    from sqair_amd.model import Model, SqairCore
    from tests.hip_util import draw_noise, params32
    from sqair_amd.data import make_sequences, to_float
    hw, T, B, K, N = (151, 256), 2, 1, 2, 2
    F = make_flags(k_particles=K, n_steps_per_image=N)
    d = make_sequences(B, T=T, canvas=hw, seed=1)
    obs = to_float(d["imgs"])
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 0, 0.05, obs.mean((0, 1))))
    m = Model(obs, None, core, K, presence=d["nums"])
    m.run(noise=draw_noise(np.random.default_rng(0), T, B * K, N, 55))
    assert np.isfinite(float(m.elbo_iwae))
    with pytest.raises(Exception, match="38 ?400|pixels|frame"):
        with core.on_stream():
            core.forward(train=True)


@pytest.mark.parametrize("batch", [0, 128])
def test_full_size_gradient_is_the_mean_of_shard_gradients(batch):
    """BASELINE configs[1] / configs[2] shape (T10, 50x50, B32, K5, N4): the gradient of the full batch equals the mean
    of the gradients of its two 16-sequence shards run as separate problems on the same noise rows — the identity the
    data-parallel training step relies on (all-reduce(sum) / world == reduce_mean over the global batch,
    sqair/model.py:91-93, sqair/targets.py:75).  With 128 sequences the full batch and its 64-sequence shards run on DIFFERENT
    kernel variants (640 against 320 particle rows: slot tail as its own launch / fused with two column tiles per workgroup;
    25 600 against 12 800 decoder rows: other tiles of the LDS-tiled kernel): the identity must hold across them."""
    from sqair_amd.data import config_inputs
    from sqair_amd.dist import shard_batch, shard_noise
    from sqair_amd.model import Model, SqairCore
    from tests.hip_util import draw_noise, params32
    ov, obs, _, _ = config_inputs(2, B=batch) if batch else config_inputs(2)
    F = make_flags(**ov)
    K, N = int(F.k_particles), int(F.n_steps_per_image)
    hw = obs.shape[2:4]
    T, B = obs.shape[:2]
    P = params32(F, hw, 1, 0.02, obs.mean((0, 1)))
    noise = draw_noise(np.random.default_rng(5), T, B * K, N, 55)

    def grad_of(o, nz):
        core = SqairCore(F, hw)
        core.set_params(P)
        Model(o, None, core, K, outputs="minimal")
        with core.on_stream():
            core.noise.copy_(torch.as_tensor(nz).reshape(core.noise.shape))
            g = core.grad_step(use_graph=True).clone()
            target = float(core.scalars[2])
        core.stream.synchronize()
        return g, target

    g_full, t_full = grad_of(obs, noise)
    parts = [grad_of(shard_batch(obs, r, 2), shard_noise(noise, K, r, 2)) for r in range(2)]
    g_mean = 0.5 * (parts[0][0] + parts[1][0])
    assert abs(0.5 * (parts[0][1] + parts[1][1]) - t_full) <= 1e-5 * abs(t_full)
    scale = float(g_full.abs().max())
    assert torch.isfinite(g_full).all() and scale > 0
    assert float((g_full - g_mean).abs().max()) <= 2e-4 * scale


def test_full_backward_cfg2_sub_batch_against_oracle():
    """Headline shape in T, K, N and frame size (T10, 50x50, K5, N4) on an 8-sequence sub-batch: every parameter's gradient
    against autograd through the fp64 oracle."""
    report, ref, _ = full_backward_case(K=5, N=4, T=10, B=8, hw=(50, 50), seed=1236)
    assert float(ref.prop_pres.detach().sum()) > 0
    check_report(report)


def test_trainer_follows_the_sequence_length_curriculum():
    """seq_len / stage_itr curriculum (mnist_tools.py:80-92): the feed hands out longer sequences as training proceeds and
    the trainer re-binds its buffers (and re-captures the gradient graph) for the new T."""
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.dataio import MinibatchFeed
    from sqair_amd.model import Model, SqairCore
    from sqair_amd.train import Trainer, curriculum_seq_len
    from tests.hip_util import params32
    K, N, B, hw = 2, 2, 4, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N, learning_rate=1e-4, seq_len=2, stage_itr=2)
    d = make_sequences(8, T=4, canvas=hw, seed=4)
    feed = MinibatchFeed(dict(imgs=to_float(d["imgs"]), nums=d["nums"], coords=d["coords"]), B, shuffle=True, seed=0,
                         seq_len=F.seq_len, stage_itr=F.stage_itr)
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 4, 0.05, to_float(d["imgs"]).mean((0, 1))))
    tr = Trainer(Model(to_float(d["imgs"][:2, :B]), None, core, K, outputs="minimal"), F)
    seen = []
    for it in range(6):
        batch = feed.next(it)
        assert batch["imgs"].shape[0] == curriculum_seq_len(F, it, 4)
        tr.step(obs=batch["imgs"], generator=torch.Generator(device="cuda").manual_seed(it))
        seen.append(core.T)
    core.stream.synchronize()
    assert seen == [2, 2, 3, 3, 4, 4]
    assert torch.isfinite(core.flat).all()


@pytest.mark.parametrize("K,N,T,B,hw", [(2, 8, 2, 2, (50, 50)), (64, 1, 2, 1, (50, 50)), (2, 1, 1, 1, (50, 50))])
def test_edges_of_the_supported_range_forward_and_backward(K, N, T, B, hw):
    """N = 8 slots (SQ_MAXN), K = 64 particles, the smallest problem (one slot, one frame, one sequence): outputs and every
    parameter gradient against the fp64 oracle."""
    report, ref, core = full_backward_case(K, N, T, B, hw, seed=31)
    check_report(report)
    lw = core.out["log_weights_per_timestep"].cpu().numpy()
    want = ref.log_weights_per_timestep.detach().numpy()
    assert np.abs(lw - want).max() <= 1e-4 * np.abs(want).max()


def test_rccl_all_reduce_on_the_gradient_buffer_single_rank():
    """The step's collective through torch.distributed's RCCL backend, issued while the core's stream is the current
    stream (world size 1 on this box: the reduction is the identity, what is checked is that the call composes with the
    one-stream discipline and the replayed gradient graph)."""
    import torch.distributed as dist
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.model import Model, SqairCore
    from tests.hip_util import params32
    if dist.is_initialized():
        pytest.skip("process group already initialised")
    K, N, T, B, hw = 2, 2, 2, 2, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N)
    obs = to_float(make_sequences(B, T=T, canvas=hw, seed=2)["imgs"])
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 4, 0.05, obs.mean((0, 1))))
    Model(obs, None, core, K, outputs="minimal")
    dist.init_process_group(backend="nccl", init_method="tcp://127.0.0.1:29617", world_size=1, rank=0)
    try:
        with core.on_stream():
            core.draw_noise(seed=3, step=0)
            g = core.grad_step(use_graph=True)
            before = g.clone()
            dist.all_reduce(g, op=dist.ReduceOp.SUM)
            g.div_(dist.get_world_size())
            after = g.clone()
            again = core.grad_step(use_graph=True).clone()   # (overwrites the same flat gradient buffer)
        core.stream.synchronize()
        assert torch.equal(after, before)
        assert float((again - before).abs().max()) <= 1e-5 * float(before.abs().max())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("options", [None, {"slot_chain": 1}], ids=["launches", "slot_chain"])
def test_gradients_match_the_golden_fixture(options):
    """(also with the forward pass of the gradient evaluation on the in-launch slot chain: the tape the adjoint reads is then the
    chain's)  tests/golden/k5_iwae_vimco_grads.npz (autograd through the fp64 oracle on the k5_iwae_vimco fixture; digest per
    parameter: sampled elements + sum / sum|.| / L2 / max|.|): the HIP backward pass on the same frames, parameters, noise."""
    import os
    from sqair_amd.model import Model, SqairCore
    from tests.hip_util_cpu import GOLDEN, fixture_params
    z = np.load(os.path.join(GOLDEN, "k5_iwae_vimco.npz"))
    g = np.load(os.path.join(GOLDEN, "k5_iwae_vimco_grads.npz"))
    assert str(g["params_sha256"]) == str(z["params_sha256"])
    T, B, K, N, H, W, _, _ = [int(v) for v in z["meta"]]
    F = make_flags(k_particles=K, n_steps_per_image=N)
    P = fixture_params(z, F, (H, W))
    core = SqairCore(F, (H, W), options=options)
    core.set_params(P)
    m = Model(z["obs"], None, core, K, presence=z["nums"], outputs=["log_weights_per_timestep", "discrete_log_prob", "presence"])
    with core.on_stream():
        core.noise.copy_(torch.as_tensor(z["noise"]).reshape(core.noise.shape))
        core.forward(train=True)
        core.backward()
    core.stream.synchronize()
    if options:
        core.check_chain(train=True)
    assert np.array_equal(core.out["presence"].cpu().numpy(), z["out_presence"].astype(np.float32))
    assert abs(float(core.scalars[2]) - float(g["vimco_target"])) <= 1e-4 * abs(float(g["vimco_target"]))
    report = []
    gmax = max(float(g[k][3]) for k in g.files if k.startswith("stat/"))
    for name, got in core.grads_by_name().items():
        got = got.cpu().numpy().astype(np.float64).reshape(-1)
        stat = g["stat/" + name]
        scale = max(float(stat[3]), 1e-4 * gmax)
        report.append((name, float(np.abs(got[g["idx/" + name]] - g["val/" + name]).max()), float(stat[3])))
        # whole-tensor digests: the L2 norm to the same relative bar
        assert abs(np.sqrt((got * got).sum()) - stat[2]) <= LOOSE * max(stat[2], scale), name
    check_report(report)


def test_l2_term_of_the_target_and_its_gradient():
    """targets.l2_reg (sqair/targets.py:31-35): weight * sum_v tf.nn.l2_loss(v) = weight * 0.5 * sum theta^2 over ALL
    trainable variables, added to the VIMCO target (model.py:160); its gradient is weight * theta (sqair_add_l2_grad)."""
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.model import Model, SqairCore
    from sqair_amd.train import Optimizer
    from tests.hip_util import draw_noise, params32
    K, N, T, B, hw = 2, 2, 2, 2, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N)
    obs = to_float(make_sequences(B, T=T, canvas=hw, seed=3)["imgs"])
    core = SqairCore(F, hw)
    core.set_params(params32(F, hw, 2, 0.05, obs.mean((0, 1))))
    m = Model(obs, None, core, K, outputs="minimal")
    noise = draw_noise(np.random.default_rng(1), T, B * K, N, 55)
    opt = Optimizer(core)
    with core.on_stream():
        core.noise.copy_(torch.as_tensor(noise).reshape(core.noise.shape))
    m._ran = True    # keep this noise
    t0, gv0 = m.make_target(opt, l2_reg=0.0)
    g0 = core.flat_grad.clone()
    l2 = 0.37
    t1, gv1 = m.make_target(opt, l2_reg=l2)
    theta = core.flat.cpu().numpy().astype(np.float64)
    assert abs(float(t1) - (float(t0) + l2 * 0.5 * float((theta * theta).sum()))) <= 1e-5 * abs(float(t1))
    want = g0.cpu().numpy().astype(np.float64) + l2 * theta
    assert np.abs(core.flat_grad.cpu().numpy() - want).max() <= 1e-5 * np.abs(want).max()
    assert len(gv1) == len(core.spec)
