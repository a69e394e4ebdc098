"""-m gpu: the whole path AWAY FROM INITIALISATION.

Every other parity suite runs at freshly initialised parameters, where the latents sit in one narrow corner: glimpse scales of
0.33 ... 0.71, centred glimpses, posterior scales far above their floors, presence logits below 6, a canvas below 0.75.  Here the
same helpers and the same bars run with a few heads of the parameters edited (tests/latent_regimes.py: EDITS) so that the ORACLE
visits what a trained or diverging model visits: magnified and minified glimpses hanging off the frame, the 1e-4 clamp of the glimpse
scale, where / what scales at their floors, live Bernoullis whose fp32 sigmoid is exactly 1, a canvas above 2, a propagation prior
with floored scales.  Every leg first REQUIRES, from the oracle's outputs alone, that it reaches the regime it is named after, and
only then compares.  The cases, sizes, seeds and edits are the one table of tests/latent_regimes.py; tests/test_latent_regimes.py
proves on the CPU that each reaches its regime, is decision-stable, and -- for the "tight" cases -- that the fp32 oracle is within
a quarter of the bars used here, which are the other suites' own: discrete outputs exact, outputs 5e-4 scaled, bounds 1e-4
relative, gradients TIGHT / LOOSE, bit identity between executors.

The two "measured" edits (`where_spread`, `tiny_scale`) are ill conditioned in fp32 whatever the implementation.  There every
quantity is judged at max(the existing bar, 4 x the fp32 oracle's own distance from the fp64 oracle), that distance measured here on
the same inputs -- the rule tests/test_presence_paths.py applies to elbo_iwae.

A gradient leg also requires a KINK-STABLE draw (tests/latent_regimes.py: kink_recorder): no bilinear sample coordinate of the oracle
within 4 fp32 ulps of an integer, where the sampler's derivative jumps and the fp64 oracle's side need not be an fp32
implementation's.  The first device run of this file had such a draw (a crop row at 15 + 2.7e-7 pixels): with a learning signal
in the thousands it moved whole gradients by 1e-2, and a 2e-6 pixel nudge of the ORACLE reproduced the kernel's figures.

Measured figures of these cases: profiles/latent_regimes_parity.json (written where SQAIR_PARITY_DIR points, nowhere otherwise)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import Model, SqairCore
from tests import latent_regimes as LR
from tests.hip_util import rel_err, run_hip, run_oracle
from tests.stream_cases import ORACLE_HW, chunk_two_case, filter_case, rollout_case
from tests.stream_harness import chunked, compare, one_pass, switches
from tests.pass_cases import (LOOSE, REL, TIGHT, check_report, full_backward_case, full_backward_inputs, live_oracle_case, live_oracle_inputs,
                              spec_launches)

pytestmark = pytest.mark.gpu

PARITY_DIR_ENV = "SQAIR_PARITY_DIR"
FP32_FACTOR = 4.0     # a "measured" quantity may be this many times as far from the fp64 oracle as the fp32 oracle is
assert (TIGHT, LOOSE, REL) == (LR.GRAD_TIGHT, LR.GRAD_LOOSE, LR.BOUND_BAR)


def _record(section, case, **figures):
    """With SQAIR_PARITY_DIR set, appends the case's measured figures to latent_regimes_parity.json there (the copy under
    profiles/ is such a file); without it nothing is written."""
    where = os.environ.get(PARITY_DIR_ENV)
    if not where:
        return
    path = os.path.join(where, "latent_regimes_parity.json")
    try:
        os.makedirs(where, exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {})[case] = dict(build_id=_capi.build_id(), **figures)
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _sig(d):
    return {k: float("%.3g" % v) for k, v in sorted(d.items())}


# ---- forward ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _forward_inputs(case):
    """The oracle side of a forward case, computed once and shared by the legs that run it (nothing in it is written to)."""
    K, N, T, B, hw, flags, edits, need = LR.FORWARD[case]
    F = make_flags(k_particles=K, n_steps_per_image=N, **flags)
    x = live_oracle_inputs(F, hw, T, B, edits=edits)
    cfg = O.make_cfg(F, hw)
    x["regimes"] = LR.counts_of(x["ref"].outputs, cfg)
    print(LR.table(x["regimes"]))
    x["prior"] = LR.prior_counts(x["P"], cfg, x["obs"], x["noise"], x["d"]["nums"]) if "floored_prior" in edits else None
    return F, x


def _require_forward(case):
    F, x = _forward_inputs(case)
    LR.require(x["regimes"], **LR.FORWARD[case][7])
    if x["prior"] is not None:
        LR.require_prior(x["prior"], **LR.PRIOR_REACH)
    return F, x


def _hip_errors(m, ref):
    """(per-output scaled errors, bound errors) of a HIP model against an oracle model, in `check_against`'s scalings."""
    out = {}
    for k, v in ref.outputs.items():
        if not k.startswith("_") and k in m.outputs:
            want = v.numpy()
            got = m.outputs[k].cpu().numpy().reshape(want.shape)
            out[k] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1.0))
    bound = {k: rel_err(getattr(m, k).cpu().numpy(), getattr(ref, k).numpy()) for k in LR.VECTORS}
    for k in LR.SCALARS:
        want = float(getattr(ref, k))
        bound[k] = abs(float(getattr(m, k)) - want) / max(abs(want), 1.0)
    return out, bound


def _check_measured_forward(case, m, ref, r32):
    """A "measured" case: discrete outputs exact; every other quantity at max(its bar, 4 x the fp32 oracle's own distance)."""
    assert LR.same_decisions(r32, ref), "the fp32 oracle must make the fp64 oracle's decisions"
    for k in ("presence", "prop_pres", "disc_pres", "obj_id", "num_steps_per_sample"):
        assert np.array_equal(getattr(m, k).cpu().numpy(), getattr(ref, k).numpy().astype(np.float32)), k
    out, bound = _hip_errors(m, ref)
    d_out, d_bound = LR.output_distances(r32, ref), LR.bound_distances(r32, ref)
    bars_out = {k: max(LR.OUTPUT_BAR, FP32_FACTOR * d_out[k]) for k in out}
    bars_bound = {k: max(LR.BOUND_BAR, FP32_FACTOR * d_bound[k]) for k in bound}
    for k in sorted(out, key=lambda k: -out[k] / bars_out[k])[:5]:
        print("{}: {:28s} fp32 oracle {:.2e}  bar {:.2e}  HIP {:.2e}".format(case, k, d_out[k], bars_out[k], out[k]))
    bad = {k: (v, bars_out[k]) for k, v in out.items() if v > bars_out[k]}
    bad.update({k: (v, bars_bound[k]) for k, v in bound.items() if v > bars_bound[k]})
    _record("forward_measured", case, fp32_oracle_distance=_sig(dict(d_out, **d_bound)), bar=_sig(dict(bars_out, **bars_bound)),
            hip_error=_sig(dict(out, **bound)))
    assert not bad, bad


@pytest.mark.parametrize("case", sorted(LR.FORWARD))
def test_forward_in_the_regime(case):
    """Every output against the fp64 oracle: presence, ids and step counts exact, every output at 5e-4 scaled, the bounds at 1e-4
    relative (`live_oracle_case`); the measured cases by the rule in this file's docstring."""
    K, N, T, B, hw, flags, edits, need = LR.FORWARD[case]
    F, x = _require_forward(case)
    if LR.conditioning(edits) == "measured":
        r32 = run_oracle(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"], dtype=torch.float32)
        m = run_hip(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"])
        _check_measured_forward(case, m, x["ref"], r32)
    else:
        m, _ = live_oracle_case(F, hw=hw, T=T, B=B, inputs=x)
    assert (m.core.lib is _capi.lib(_capi.WIDE_LIB_PATH)) == ("n_what" in flags)
    out, bound = _hip_errors(m, x["ref"])
    worst = max(out, key=out.get)
    print("{}: worst output {} {:.2e}, worst bound {:.2e}".format(case, worst, out[worst], max(bound.values())))
    # (the bars of a measured case, each with the fp32 oracle's distance it came from: section `forward_measured`)
    _record("forward", case, edits=list(edits), conditioning=LR.conditioning(edits), output_bar=LR.OUTPUT_BAR, bound_bar=LR.BOUND_BAR,
            oracle_margin=x["margin"], regimes=x["regimes"], prior=x["prior"], worst_scaled_abs_err=out[worst], worst_output=worst,
            worst_bound_err=max(bound.values()), hip_error=_sig(dict(out, **bound)), elbo_iwae=float(x["ref"].elbo_iwae))


def _outs(m):
    return dict({k: v.detach().cpu().numpy().copy() for k, v in m.core.out.items()}, log_weights=m.core.log_weights.cpu().numpy().copy())


@pytest.mark.parametrize("case", LR.EXECUTORS)
def test_executors_agree_in_the_regime(case):
    """The in-launch slot chain and the specialised instantiations (these cases have the shipped shape: they take them) against
    the plain generic launches on the same inputs: every output bit for bit, eager and as a graph replay; the slot chain itself
    held against the oracle at the forward bars."""
    K, N, T, B, hw, flags, edits, need = LR.FORWARD[case]
    F, x = _require_forward(case)
    run = lambda options, use_graph=False: run_hip(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"], options=options,
                                                   use_graph=use_graph)
    n0 = spec_launches()
    ref = _outs(run({"specialised": 0}))
    assert spec_launches() == n0
    assert np.array_equal(ref["prop_pres"], x["ref"].prop_pres.numpy()) and np.array_equal(ref["disc_pres"], x["ref"].disc_pres.numpy())
    for name, options, use_graph in (("specialised", {"specialised": 1}, False), ("specialised, graph", {"specialised": 1}, True),
                                     ("slot_chain", {"slot_chain": 1}, False), ("slot_chain, graph", {"slot_chain": 1}, True),
                                     ("slot_chain, generic", {"slot_chain": 1, "specialised": 0}, False)):
        n0 = spec_launches()
        got = _outs(run(options, use_graph))
        if "slot_chain" not in options:
            assert spec_launches() - n0 > 0, name
        assert set(got) == set(ref)
        for k, v in ref.items():
            assert np.array_equal(v, got[k], equal_nan=True), (case, name, k)
    if LR.conditioning(edits) == "tight":
        live_oracle_case(F, hw=hw, T=T, B=B, inputs=x, options={"slot_chain": 1})


def test_forward_graph_replay_equals_eager_in_the_regime():
    case = LR.GRAPH_FORWARD
    K, N, T, B, hw, flags, edits, need = LR.FORWARD[case]
    F, x = _require_forward(case)
    eager = _outs(run_hip(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"]))
    m = run_hip(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"], use_graph=True)
    assert m.core.graph_nodes() > 100
    replay = _outs(m)
    for k, v in eager.items():
        assert np.array_equal(v, replay[k], equal_nan=True), k


# ---- backward --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _backward_inputs(edits, flags_items):
    """The oracle side of a backward case (differentiated once, by the first leg that runs it), shared by its executors."""
    inputs = full_backward_inputs(3, 3, 3, 3, LR.BWD_HW, LR.BWD_SEED, dict(flags_items), edits, seed0=LR.bwd_noise_seed0(edits))
    F, obs, P, noise, ref, orc = inputs
    cfg = O.make_cfg(F, LR.BWD_HW)
    ref.regimes = LR.counts_of(ref.outputs, cfg)
    print(LR.table(ref.regimes))
    ref.prior = LR.prior_counts(P, cfg, obs, noise) if "floored_prior" in edits else None
    ref.kinks = LR.kink_clearance(P, cfg, obs, noise)
    return inputs


def _require_backward(case):
    K, N, T, B, flags, options, wide, edits, need = LR.BACKWARD[case]
    inputs = _backward_inputs(edits, tuple(sorted(flags.items())))
    ref = inputs[4]
    LR.require(ref.regimes, **need)
    if ref.prior is not None:
        LR.require_prior(ref.prior, **LR.PRIOR_REACH)
    # ... and that the draw is kink-stable: no bilinear sample coordinate of the oracle within KINK_ULPS fp32 ulps of an integer, where
    # the sampler's derivative jumps and the oracle's side need not be an fp32 implementation's (tests/latent_regimes.py)
    assert ref.kinks.clearance >= 1.0, ref.kinks.closest()
    return inputs


def _fp32_gradient_distance(inputs):
    F, obs, P, noise, ref, orc = inputs
    o32 = O.SqairOracle(P, O.make_cfg(F, LR.BWD_HW), torch.float32, requires_grad=True)
    r32 = o32.model(obs, noise)
    assert LR.same_decisions(r32, ref), "the fp32 oracle must make the fp64 oracle's decisions"
    o32.make_target(r32).backward()
    return LR.gradient_rel(LR.gradient_report(LR.oracle_grads(o32), LR.oracle_grads(orc)))


@pytest.mark.parametrize("case", sorted(LR.BACKWARD))
def test_full_backward_in_the_regime(case):
    """Every parameter's gradient against autograd through the fp64 oracle at the bars of tests/pass_cases.py: TIGHT, and
    LOOSE for the two `*.transform.scale_offset` scalars (`check_report`); the measured cases per parameter at max(that bar, 4 x the
    fp32 oracle's own distance).

    The clamp cases additionally compare the two SCALE entries of `disc.transform.l2.b` one by one: every discovered glimpse's
    scale is below the 1e-4 clamp there, the inverse transformer's grid divides by it, and the clamp's own gradient path contributes
    nothing at the bar's resolution (tests/latent_regimes.py: CLAMP_CONTRIBUTION; measured on the oracle by
    tests/test_latent_regimes.py) -- so a kernel whose adjoint blows up through 1 / sc, or that loses the gradient that reaches
    these entries through the log-probabilities, fails here."""
    K, N, T, B, flags, options, wide, edits, need = LR.BACKWARD[case]
    inputs = _require_backward(case)
    orc = inputs[5]
    report, ref, core = full_backward_case(K, N, T, B, LR.BWD_HW, LR.BWD_SEED, flags=flags, options=options, edits=edits, inputs=inputs)
    assert (core.lib is _capi.lib(_capi.WIDE_LIB_PATH)) == wide
    rel = LR.gradient_rel(report)
    worst = max(rel, key=rel.get)
    figures = dict(edits=list(edits), conditioning=LR.conditioning(edits), tight=TIGHT, loose=LOOSE, regimes=ref.regimes, prior=ref.prior,
                   worst_rel_err=rel[worst], worst_parameter=worst)
    base = {n: (LOOSE if n in LR.GRAD_LOOSE_NAMES else TIGHT) for n in rel}
    if LR.conditioning(edits) == "measured":
        dist = _fp32_gradient_distance(inputs)
        bars = {n: max(base[n], FP32_FACTOR * dist[n]) for n in rel}
        for n in sorted(rel, key=lambda n: -rel[n] / bars[n])[:8]:
            print("{}: {:34s} fp32 oracle {:.2e}  bar {:.2e}  HIP {:.2e}".format(case, n, dist[n], bars[n], rel[n]))
        bad = {n: (rel[n], bars[n]) for n in rel if not np.isfinite(rel[n]) or rel[n] > bars[n]}
        _record("backward", case, fp32_oracle_distance=_sig(dist), bar=_sig(bars), hip_error=_sig(rel), **figures)
        assert not bad, bad
    else:
        _record("backward", case, bar=_sig(base), hip_error=_sig(rel), **figures)
        check_report(report)
    if case in LR.CLAMP_CASES:
        want = orc.P["disc.transform.l2.b"].grad.numpy()
        got = core.grads_by_name()["disc.transform.l2.b"].cpu().numpy().reshape(want.shape)
        gmax = max(s for _, _, s in report)
        bar = TIGHT * max(float(np.abs(want).max()), 1e-4 * gmax)
        print("{}: d / d disc.transform.l2.b[:2] oracle {} HIP {} bar {:.3e}".format(case, want[:2], got[:2], bar))
        _record("clamp", case, oracle=[float(v) for v in want[:2]], hip=[float(v) for v in got[:2]], bar=bar)
        assert np.isfinite(got).all() and (np.abs(got[:2] - want[:2]) <= bar).all()


def test_training_graph_replay_equals_eager_in_the_regime():
    """forward(train) + ELBO + backward replayed as one HIP graph gives the eager gradients (the bar of
    tests/test_hip_backward.py: 1e-5 of the largest gradient; float atomics leave the order of additions free), at the combined
    edit."""
    inputs = _require_backward(LR.GRAPH_TRAIN)
    F, obs, P, noise, ref, orc = inputs
    core = SqairCore(F, LR.BWD_HW)
    core.set_params(P)
    Model(obs, None, core, int(F.k_particles), outputs="minimal")
    core.noise.copy_(torch.as_tensor(noise).reshape(core.noise.shape))
    g0 = core.grad_step(use_graph=False).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g0).all())
    for _ in range(2):
        g1 = core.grad_step(use_graph=True).clone()
        torch.cuda.synchronize()
        assert core.train_graph_nodes > 100
        assert float((g1 - g0).abs().max()) <= 1e-5 * float(g0.abs().max())


# ---- stream, carried training chunk, particle filter, forecast -------------------------------------------------------------------------
def test_stream_chunks_equal_the_single_pass_in_the_regime():
    """A 12-frame sequence at the combined edit fed in chunks of 1 and of 4 frames with the state carried: bit for bit the single
    pass; and the single pass itself against the oracle at the forward bars."""
    c = LR.STREAM
    K, N, T, B, hw = c["K"], c["N"], c["T"], c["B"], c["hw"]
    F = make_flags(k_particles=K, n_steps_per_image=N)
    x = live_oracle_inputs(F, hw, T, B, edits=c["edits"])
    counts = LR.counts_of(x["ref"].outputs, O.make_cfg(F, hw))
    print(LR.table(counts))
    LR.require(counts, **c["minimums"])
    m, _ = live_oracle_case(F, hw=hw, T=T, B=B, inputs=x)
    core = SqairCore(F, hw)
    core.set_params(x["P"])
    whole = one_pass(core, x["obs"], x["noise"])
    assert np.array_equal(whole["presence"], x["ref"].presence.numpy()) and np.array_equal(whole["obj_id"], x["ref"].obj_id.numpy().astype(np.float32))
    for sizes in c["chunks"]:
        enc, dec = switches(T, list(sizes), B, B * K, N, hw)
        assert not enc and not dec, "the shapes of this case keep every once-per-pass layer on one kernel"
        got, _ = chunked(core, x["obs"], x["noise"], list(sizes))
        compare(got, whole)
    out, bound = _hip_errors(m, x["ref"])
    _record("stream", "single_pass_T12", regimes=counts, worst_scaled_abs_err=max(out.values()), worst_output=max(out, key=out.get),
            worst_bound_err=max(bound.values()))


def test_stream_training_chunk_in_the_regime():
    """The chunk-two case of tests/test_stream_train.py (imported rows, one lane reset, every gradient against tests/tbptt_ref.py at
    that file's bar) at the combined edit; chunk 2 must reach the regime on the oracle, on a kink-stable draw."""
    c = LR.STREAM_TRAIN
    cfg = O.make_cfg(make_flags(**c["flags"]), ORACLE_HW)

    def require(out1, out2):
        counts = LR.counts_of(out2, cfg)
        print("chunk 2:", LR.table(counts))
        LR.require(counts, **c["minimums"])
        # (every oracle pass of the case up to here, the rejected draws included: the differentiated chunk's coordinates are among them)
        assert kinks.clearance >= 1.0, kinks.closest()

    with LR.kink_recorder() as kinks:
        chunk_two_case(c["flags"], None, False, require=require, edits=c["edits"])


def test_smc_evidence_at_saturated_logits():
    """SqairStream(resample="systematic") against the fp64 particle filter of tests/smc_ref.py (tests/test_smc_oracle.py's case
    `gru` and all its bars: outputs, log weights, the evidence, decisions and ancestors) with every live presence logit beyond 17;
    every step's proposal must hold such Bernoullis on the oracle."""
    c = LR.SMC
    cfg = O.make_cfg(make_flags(**c["flags"]), ORACLE_HW)
    seen = []

    def require(outputs, step):
        counts = LR.counts_of(outputs, cfg)
        seen.append(counts["saturated_logit"])
        LR.require(counts, **c["minimums"])

    n, worst = filter_case("saturated_presence", c["flags"], c["B"], c["frames_per_step"], c["frames"], c["ess_frac"], False,
                            edits=c["edits"], require=require)
    _record("smc", "saturated_presence", saturated_logits_per_step=seen, counts=n, worst=_sig(worst))


def test_forecast_at_the_floored_prior():
    """A forecast against the fp64 rollout of tests/forecast_ref.py at tests/test_forecast.py's gate, with the propagation prior's
    scales at their floor and its presence logit saturated -- required of the reference rollout's OWN priors (every forecast frame
    samples from them) before the device runs."""
    c = LR.FORECAST
    seen = {}

    def require(ref, state):
        seen.update(LR.forecast_prior_counts(ref))
        print("forecast priors:", seen)
        LR.require_prior(seen, **c["minimums"])

    got, ref = rollout_case("floored_prior", c["flags"], c["hw"], c["B"], c["S"], c["Fn"], require=require, edits=c["edits"])
    assert float(got["presence"][-1].sum()) >= 4
    _record("forecast", "floored_prior", prior=dict(seen))
