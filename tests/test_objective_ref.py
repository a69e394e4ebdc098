"""No GPU: tests/objective_ref.py pinned -- hand-known answers, the oracle's control variate against its brute-force definition, the
restatement against the oracle in float64 -- and the power check over the case list of tests/test_objective_kernels.py and
tests/test_optimiser_kernels.py: every mistake of MUTATIONS / OPT_MUTATIONS, made in the float32 restatement, exceeds the bar of at
least one output in at least one case of the GPU test, in the GPU test's own metric; the unmutated restatement is under every bar."""
import math

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd.train import rmsprop_reference
from tests import objective_ref as OR
from tests import slot_adjoint_ref as R

F32, F64 = np.float32, np.float64


def _ref(LW, reinforce=0, dl=None, xs=()):
    """reference() of one frame: LW [B, K]."""
    LW = np.asarray(LW, F32)
    return OR.reference(LW[None], None if dl is None else np.asarray(dl, F32)[None], [np.asarray(x, F32)[None] for x in xs], reinforce)


# ------------------------------------------------------------------------------------------------ hand-known answers
@pytest.mark.parametrize("K", [2, 5, 64, 100])
def test_bit_equal_lane(K):
    lw = F32(-123.456)
    r = _ref(np.full((3, K), lw))
    assert np.allclose(r["elbo_per_ex"], float(lw), rtol=0, atol=1e-12) and np.allclose(r["iw"], 1.0 / K, rtol=1e-14)
    assert abs(r["scalars"][3] - K) < 1e-10 * K and np.abs(r["signal"]).max() < 1e-11      # control variate = lw
    assert abs(r["scalars"][0] - float(lw)) < 1e-12 and abs(r["scalars"][1] - float(lw)) < 1e-12


def test_two_particles_control_variate_is_the_other_log_weight():
    rng = np.random.default_rng(0)
    LW = rng.normal(-50, 5, (7, 2)).astype(F32)
    r = _ref(LW)
    assert np.allclose(r["signal"], LW.astype(F64) - LW.astype(F64)[:, ::-1], rtol=0, atol=1e-12)


def test_one_particle_200_nats_above():
    K = 5
    LW = np.full((1, K), -300.0, F32)
    LW[0, 3] = -100.0
    r = _ref(LW)
    assert abs(r["scalars"][3] - 1.0) < 1e-12
    assert np.allclose(r["iw"][0], np.eye(K)[3], rtol=0, atol=1e-80)
    assert abs(r["elbo_per_ex"][0] - (-100.0 - math.log(K))) < 1e-12


def test_one_particle():
    LW, dl = np.array([[-7.5], [3.25]], F32), np.array([[-2.0], [-1.0]], F32)
    v, rf = _ref(LW, 0, dl), _ref(LW, 1, dl)
    assert np.isnan(v["signal"]).all() and np.isnan(v["scalars"][2]) and np.isfinite(np.delete(v["scalars"], 2)).all()
    assert np.array_equal(v["elbo_per_ex"], LW[:, 0].astype(F64)) and np.array_equal(v["iw"], np.ones((2, 1)))
    assert np.array_equal(rf["signal"], LW.astype(F64)) and np.isfinite(rf["scalars"]).all()
    assert abs(rf["scalars"][2] - np.mean(-LW[:, 0].astype(F64) - LW[:, 0].astype(F64) * dl[:, 0])) < 1e-12


def test_importance_weighted_mean_and_gradients():
    rng = np.random.default_rng(1)
    T, B, K = 3, 4, 5
    lw_t, dl_t = rng.normal(-5, 2, (T, B, K)).astype(F32), rng.normal(-3, 2, (T, B, K)).astype(F32)
    x = rng.standard_normal((T, B, K)).astype(F32)
    for reinforce in (0, 1):
        r = OR.reference(lw_t, dl_t, [x], reinforce)
        w = r["iw"]
        assert abs(r["means"][0] - np.mean((w * x.astype(F64).mean(0)).sum(-1))) < 1e-14
        assert np.allclose(r["g_log_w_t"], np.broadcast_to(-w / (B * T), (T, B, K)), rtol=1e-12, atol=0)
        assert np.allclose(r["g_disc_lp_t"], np.broadcast_to(-r["signal"] / (B * K * T), (T, B, K)), rtol=1e-12, atol=0)
    # disc_lp_t NULL is disc_lp_t = 0: the target loses its signal term, the gradient with respect to it stays -signal / (B K T)
    a, b = OR.reference(lw_t, None, [], 0), OR.reference(lw_t, np.zeros_like(lw_t), [], 0)
    assert all(np.array_equal(a[k], b[k]) for k in a) and abs(a["scalars"][2] + a["scalars"][1] / T) < 1e-14


# ------------------------------------------------------------------------------------------------ the control variate, independently
@pytest.mark.parametrize("K", [2, 3, 13, 70])
def test_control_variate_against_its_brute_force_definition(K):
    rng = np.random.default_rng(K)
    for regime in OR.REGIMES:
        lw = OR.draw_lane(rng, regime, 3, K).astype(F32).astype(F64).sum(0)
        got = O.vimco_control_variate(torch.tensor(lw)[None]).numpy()[0]
        for k in range(K):
            v = lw.copy()
            v[k] = math.fsum(np.delete(lw, k)) / (K - 1)
            m = v.max()
            want = m + math.log(math.fsum(math.exp(a - m) for a in v) / K)
            assert abs(got[k] - want) <= 1e-13 * max(1.0, np.abs(lw).max()), (regime, k)


# ------------------------------------------------------------------------------------------------ the restatement is the reference
@pytest.fixture(scope="module")
def built():
    return {name: OR.build_case(name) for name in OR.CASES}


def test_restatement_in_float64_is_the_reference(built):
    for name, c in built.items():
        r = OR.restate(c["lw_t"], c["dl_t"], c["xs"][:c["n_means"]], c["reinforce"], dt=torch.float64)
        e = OR.errors(r, c["ref"], c["scales"], c["names"] + (["g_log_w_t", "g_disc_lp_t"] if c["chained"] else []))
        assert max(e.values()) < 1e-13, (name, e)


def test_case_list_covers_its_axes(built):
    cs = list(OR.CASES.values())
    assert 38 <= len(cs) <= 44
    assert {c["K"] for c in cs} == {1, 2, 5, 13, 32, 33, 64, 65, 100, 256}
    for c in cs:
        fpi = OR.fpi_of(c["K"])
        assert c["T"] in (1, fpi, fpi + 1, 2 * fpi + 3) and c["T"] * c["B"] * c["K"] * (2 + c["n_means"]) * 4 <= 400 * 1024
    for K in {c["K"] for c in cs}:
        assert {OR.fpi_of(K) + 1, 2 * OR.fpi_of(K) + 3, OR.fpi_of(K), 1} == {c["T"] for c in cs if c["K"] == K and not c["wide"]}
    for small in (True, False):       # every value of the other axes, in k_elbo's cases and in k_elbo_wide's
        sub = [c for c in cs if (c["K"] <= 64) == small]
        assert {c["disc"] for c in sub} == {True, False} and {c["reinforce"] for c in sub} == {0, 1}
        assert {c["null"] for c in sub} == {None} | set(OR.OUTPUTS), small
    assert {c["B"] for c in cs if c["K"] <= 64} == {1, 16, 17, 33, 50} and {c["n_means"] for c in cs} == {0, 1, 3, 7, 8}
    assert {c["n_means"] for c in cs if c["K"] > 64} >= {0, 1, 3}
    assert sorted((c["K"], c["wide"]) for c in cs if c["wide"]) == [(5, True), (100, True)]
    # the chained list: every K 5, 33, 64, 100 case that passes iw and signal; both targets, disc_lp_t NULL and T = 1 among them
    chained = [OR.CASES[n] for n in OR.CHAINED]
    assert chained == [c for n, c in sorted(OR.CASES.items()) if c["K"] in (5, 33, 64, 100) and c["null"] not in ("iw", "signal")]
    assert {c["K"] for c in chained} == {5, 33, 64, 100} and {c["reinforce"] for c in chained} == {0, 1}
    assert {c["disc"] for c in chained} == {True, False} and 1 in {c["T"] for c in chained} and len(chained) >= 10
    assert {(c["reinforce"], c["disc"]) for c in chained} >= {(0, True), (0, False), (1, False)}
    # the three dealt axes are not tied to one another: a REINFORCE case with every output, disc_lp_t NULL beside several NULL outputs
    assert any(c["reinforce"] and c["null"] is None for c in cs) and len({c["null"] for c in cs if not c["disc"]}) >= 4
    assert len({(c["disc"], c["reinforce"], c["null"]) for c in cs}) >= 20
    for small in (True, False):       # iw_means_in / iw_means_out NULL with n_means = 0, on either kernel
        assert any(c["null_means"] for c in cs if (c["K"] <= 64) == small)
    assert all(c["n_means"] == 0 for c in cs if c["null_means"])
    assert sorted(t * b * k for t, b, k in OR.BWD_SHAPES) == [1, 255, 256, 257, 3 * 33 * 70]
    regimes = set()
    for c in built.values():
        regimes |= set(c["regimes"])
        if c["B"] >= 7:
            assert len(set(c["regimes"][:7])) == 7          # mixed within the batch: a lane's neighbours are in other regimes
    assert regimes == set(OR.REGIMES)
    # what the regimes promise, on the float64 reference
    seen = set()
    for c in built.values():
        for b, rg in enumerate(c["regimes"]):
            lw, iw = c["ref"]["log_weights"][b], c["ref"]["iw"][b]
            if rg == "bit_equal":
                assert np.all(lw == lw[0])
            if rg == "one_far_below" and c["K"] > 1:
                assert F32(iw.min()) == 0.0 and lw.max() - lw.min() > 150
            if rg == "two_leaders" and c["K"] > 2:
                top = np.sort(lw)[::-1]
                assert top[0] - top[1] <= 0.1 + 1e-3 and top[1] - top[2] > 40
            if rg == "near_equal" and c["K"] > 1:
                assert 1.0 / (iw ** 2).sum() > 0.9 * c["K"]
            seen.add(rg)
    assert seen == set(OR.REGIMES)


# ------------------------------------------------------------------------------------------------ the power check
def _bars(built):
    return {kernel: {k: R.bar_from_fp32(v) for k, v in OR.worst32(built, kernel).items()} for kernel in ("k_elbo", "k_elbo_wide")}


def test_unmutated_restatement_is_under_every_bar(built):
    bars = _bars(built)
    for name, c in built.items():
        for k, e in OR.mutated_errors(name, c, None).items():
            assert e <= bars[OR.kernel_of(name)][k], (name, k, e)
    print({kern: {k: "%.2e" % v for k, v in b.items()} for kern, b in bars.items()})


@pytest.mark.parametrize("kernel", ["k_elbo", "k_elbo_wide"])
@pytest.mark.parametrize("mutate", OR.MUTATIONS)
def test_gpu_cases_see_the_mistake(built, mutate, kernel):
    if kernel == "k_elbo_wide" and mutate in ("frames_after_first_chunk_dropped", "last_partial_chunk_twice", "lane_b16_gets_lane_b"):
        # k_elbo's strip loop and its two-lanes-per-trip pairing; k_elbo_wide has neither (fpi = 1 there: the first mistake is still
        # "every frame after the first", which its cases see; the other two cannot be made)
        if mutate != "frames_after_first_chunk_dropped":
            return
    bars = _bars(built)[kernel]
    for name in sorted(n for n in built if OR.kernel_of(n) == kernel):
        over = {k: (e, bars[k]) for k, e in OR.mutated_errors(name, built[name], mutate).items() if not e <= bars[k]}
        if over:
            print(mutate, "seen by", name, {k: "%.2e > %.2e" % v for k, v in over.items()})
            return
    raise AssertionError("no case of {} sees {}".format(kernel, mutate))


# ------------------------------------------------------------------------------------------------ the optimiser
def test_rms_step_in_float64_is_the_reference_and_the_first_step():
    theta, g, ms, mom = OR.rms_state(1025, 0)
    a = OR.rms_step(theta, g, ms, mom, OR.RMS_HYPER[1], 0.5)
    h = OR.RMS_HYPER[1]
    b = rmsprop_reference(theta.astype(F64), g.astype(F64) * 0.5, ms.astype(F64), mom.astype(F64), h["lr"], h["decay"], h["momentum"], h["eps"])
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.isfinite(a[0]).all() and a[2][1] == F64(OR.RMS_HYPER[1]["momentum"]) * mom[1]       # ms = 0, g = 0: 0 / sqrt(eps) = 0
    # hand-known: ms0 = 1, mom0 = 0, g = 1, the defaults -> ms = 1, mom = lr / sqrt(1 + eps)
    t1, s1, m1 = OR.rms_step(np.zeros(1), np.ones(1), np.ones(1), np.zeros(1), OR.RMS_HYPER[0], 1.0)
    assert abs(s1[0] - 1.0) < 1e-15 and abs(m1[0] - 1e-3) < 1e-12 and abs(t1[0] + 1e-3) < 1e-12


def test_rms_case_list_covers_its_axes():
    cs = list(OR.rms_cases().values())
    assert {c[0] for c in cs} == set(OR.RMS_N) and {c[1] for c in cs} == set(OR.RMS_ALIGN)
    assert {c[3] for c in cs} == set(OR.RMS_SCALES) and len({id(c[2]) for c in cs}) == 2
    for n in OR.RMS_N:
        assert {"aligned"} < {c[1] for c in cs if c[0] == n}
    for n in (3, 1025):               # each of the four buffers off in turn
        assert {c[1] for c in cs if c[0] == n} == set(OR.RMS_ALIGN)


@pytest.mark.parametrize("mutate", OR.OPT_MUTATIONS[:4])
def test_rms_cases_see_the_mistake(mutate):
    bars = {k: R.bar_from_fp32(v) for k, v in OR.rms_worst32().items()}
    print("bars", bars)
    ok = OR.rms_errors
    for i, (name, (n, al, hyper, gs)) in enumerate(OR.rms_cases().items()):
        st = OR.rms_state(n, i)
        ref = OR.rms_step(*st, hyper, gs)
        assert all(e <= bars[k] for k, e in ok(OR.rms_step(*st, hyper, gs, dt=F32), ref, st, hyper).items())
    for i, (name, (n, al, hyper, gs)) in enumerate(OR.rms_cases().items()):
        st = OR.rms_state(n, i)
        e = ok(OR.rms_step(*st, hyper, gs, dt=F32, mutate=mutate), OR.rms_step(*st, hyper, gs), st, hyper)
        if any(not v <= bars[k] for k, v in e.items()):
            print(mutate, "seen by", name, e)
            return
    raise AssertionError("no case sees " + mutate)


def test_l2_cases_see_the_mistake():
    bar = R.bar_from_fp32(OR.l2_worst32())
    theta, grad = OR.l2_state(257, 3)
    assert np.array_equal(OR.l2_step(theta, grad, 0.5), grad.astype(F64) + 0.5 * theta.astype(F64))
    seen = False
    for i, n in enumerate(OR.L2_N):
        for l2 in OR.L2_WEIGHTS:
            theta, grad = OR.l2_state(n, i)
            assert OR.l2_error(OR.l2_step(theta, grad, l2, dt=F32), theta, grad, l2) <= bar
            seen = seen or not OR.l2_error(OR.l2_step(theta, grad, l2, dt=F32, mutate="l2_on_grad"), theta, grad, l2) <= bar
    assert seen
