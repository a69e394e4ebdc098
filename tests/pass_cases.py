"""The whole-pass parity cases: a forward or a full backward pass of the HIP library against the CPU oracle on identical inputs,
parameters and a decision-stable noise draw, and the bars they are judged by.  tests/test_hip_forward.py, test_hip_backward.py and
test_hip_specialised.py state their cases with these; tests/test_presence_paths.py and test_regime_paths.py run the same cases
on other presence patterns and latent regimes, the stream training tests judge their gradients by `check_report`'s bars, and
tests/fuzz_forward.py draws random ones.  Importable without a GPU: nothing here touches the device before a case runs.

Not rewritten by pytest, so every assert here carries what it compared."""
import numpy as np
import torch

from sqair_amd import _capi
from sqair_amd.data import make_sequences, to_float
from sqair_amd.flags import make_flags
from sqair_amd.model import Model, SqairCore
from tests import presence_patterns
from tests.hip_util import draw_noise, params32, rel_err, run_hip, stable_noise

REL = 1e-4  # tolerance stated by north_star


def _same_decisions(name, got, ref):
    assert np.array_equal(got, ref), (name, got.shape, ref.shape, np.argwhere(got != ref)[:8].tolist() if got.shape == ref.shape else None)


# ------------------------------------------------------------------------------------------------ forward
def check_against(m, ref_out, ref_model, names, T, tol=5e-4, scalar_bars=None):
    # scalar_bars {name: absolute bar}: replaces REL * max(|ref|, 1) for that scalar where a case has MEASURED the fp32 rounding of the
    # quantity on the oracle itself (tests/test_presence_paths.py); every other bar is the file's own
    # discrete decisions first: exact
    for k in ("presence", "prop_pres", "disc_pres", "obj_id", "num_steps_per_sample"):
        if k in ref_out:
            _same_decisions(k, getattr(m, k).cpu().numpy(), np.asarray(ref_out[k], dtype=np.float32))
    worst = {}
    for k in names:
        got = m.outputs[k].cpu().numpy()
        ref = np.asarray(ref_out[k])
        if got.shape != ref.shape and got.shape[-1] == 1 and got.shape[:-1] == ref.shape:
            # n_steps_per_image = 1: the reference squeezes EVERY output whose last dimension is 1 before it writes it
            # (seq.py:255-257, restated by the oracle), the per-slot log-probabilities [R, 1] included; the HIP outputs keep [T, R, N]
            got = got[..., 0]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        scale = max(np.abs(ref).max(), 1.0)
        worst[k] = float(np.abs(got - ref).max() / scale)
    bad = {k: v for k, v in worst.items() if v > tol}
    assert not bad, bad
    for k in ("log_weights", "elbo_iwae_per_example"):
        err = rel_err(getattr(m, k).cpu().numpy(), ref_model[k])
        assert err < REL, (k, err, REL)
    for k in ("elbo_vae", "elbo_iwae", "data_ll", "kl", "log_p_z", "log_q_z_given_x"):
        got, ref = float(getattr(m, k)), float(ref_model[k])
        assert abs(got - ref) <= (scalar_bars or {}).get(k, REL * max(abs(ref), 1.0)), (k, got, ref)
    return worst


def live_oracle_inputs(F, hw, T, B, edits=None):
    """Frames, parameters and the decision-stable noise draw of a live-oracle case, with the oracle's result.  edits: names of
    tests/latent_regimes.EDITS applied to the initialised parameters (tests/test_regime_paths.py)."""
    K, N = int(F.k_particles), int(F.n_steps_per_image)
    d = make_sequences(B, T=T, canvas=hw, n_objects=(1, 2), obj_size=20, seed=9)
    obs = to_float(d["imgs"])
    P = params32(F, hw, 5, 0.05, obs.mean((0, 1)))
    if edits:
        from tests import latent_regimes
        P = latent_regimes.apply_edits(P, F, edits)
    # the draw is chosen on the ORACLE's own decision margin (never on the HIP result); presence must then agree exactly
    noise, ref, _, margin = stable_noise(F, hw, P, obs, T, B * K, N, nums=d["nums"], nzw=4 + int(F.n_what) + 1)
    # which slot layouts the case reaches (tests/presence_patterns.py; the cases that REQUIRE some are in tests/test_presence_paths.py)
    counts = presence_patterns.count(presence_patterns.classify_outputs(ref.outputs, N))
    print(presence_patterns.table(counts))
    return dict(d=d, obs=obs, P=P, noise=noise, ref=ref, margin=margin, counts=counts)


def live_oracle_case(F, hw=(32, 40), T=3, B=3, tol=5e-4, options=None, inputs=None, scalar_bars=None):
    x = inputs or live_oracle_inputs(F, hw, T, B)
    d, obs, P, noise, ref = x["d"], x["obs"], x["P"], x["noise"], x["ref"]
    m = run_hip(F, hw, P, obs, noise, nums=d["nums"], options=options)
    _same_decisions("prop_pres", m.prop_pres.cpu().numpy(), ref.prop_pres.numpy())
    _same_decisions("disc_pres", m.disc_pres.cpu().numpy(), ref.disc_pres.numpy())
    ref_out = {k: v.numpy() for k, v in ref.outputs.items() if not k.startswith("_")}
    ref_model = {k: getattr(ref, k).numpy() for k in ("log_weights", "elbo_iwae_per_example", "elbo_vae", "elbo_iwae",
                                                      "data_ll", "kl", "log_p_z", "log_q_z_given_x")}
    check_against(m, ref_out, ref_model, list(ref_out), T, tol, scalar_bars)
    return m, ref


def spec_launches():
    return int(_capi.lib().sqair_debug_specialised_launches())


# ------------------------------------------------------------------------------------------------ the slot chain
def chain_inputs(B, K, N, T, hw, seed=3, obj_size=None, **flags):
    """(F, d, obs, P, noise) of a case of tests/test_slot_chain.py: parameters of seed 0, the noise drawn with the data's seed."""
    F = make_flags(k_particles=K, n_steps_per_image=N, **flags)
    # (obj_size: tests/fuzz_forward.py draws canvases down to 8 x 8 -- the generator, like the reference's, re-draws a sample until
    #  its objects fit without overlap, i.e. for ever when they cannot)
    d = make_sequences(B, T=T, canvas=hw, seed=seed, **({"obj_size": obj_size} if obj_size else {}))
    obs = to_float(d["imgs"])
    P = params32(F, hw, 0, 0.05, obs.mean((0, 1)))
    noise = draw_noise(np.random.default_rng(seed), T, B * K, N, 4 + int(F.n_what) + 1)
    return F, d, obs, P, noise


def chain_run(F, hw, d, obs, P, noise, K, chain, use_graph):
    """One whole pass with the slot chain on or off: (core, model, every output on the host)."""
    core = SqairCore(F, hw, options={"slot_chain": 1} if chain else None)
    core.set_params(P)
    m = Model(obs, None, core, K, presence=d["nums"], debug=chain)   # (debug: also asserts every chain launch completed)
    m.run(noise=noise, use_graph=use_graph)
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().numpy().copy() for k, v in core.out.items()}
    out["log_weights"] = core.log_weights.cpu().numpy().copy()
    out["scalars"] = core.scalars.cpu().numpy().copy()
    return core, m, out


# ------------------------------------------------------------------------------------------------ backward
def full_backward_inputs(K, N, T, B, hw, seed, flags=None, edits=None, seed0=100):
    """CPU: flags, frames, parameters (with the named tests/latent_regimes.EDITS, if any), the decision-stable noise draw and the
    fp64 oracle's pass through it with autograd on (seed0: the first noise seed tried).  Returns (F, obs, P, noise, oracle model,
    oracle)."""
    F = make_flags(k_particles=K, n_steps_per_image=N, **(flags or {}))
    d = make_sequences(B, T=T, canvas=hw, n_objects=(1, 2), obj_size=max(2, min(28, min(hw) // 2)), seed=seed)
    obs = to_float(d["imgs"])
    P = params32(F, hw, 4, 0.05, obs.mean((0, 1)))
    if edits:
        from tests import latent_regimes
        P = latent_regimes.apply_edits(P, F, edits)
    noise, ref, orc, _ = stable_noise(F, hw, P, obs, T, B * K, N, seed0=seed0, requires_grad=True, nzw=4 + int(F.n_what) + 1)
    # which slot layouts the case reaches (tests/presence_patterns.py; the cases that REQUIRE some are in tests/test_presence_paths.py)
    ref.pattern_counts = presence_patterns.count(presence_patterns.classify_outputs(ref.outputs, N))
    print(presence_patterns.table(ref.pattern_counts))
    return F, obs, P, noise, ref, orc


def full_backward_case(K, N, T, B, hw, seed, flags=None, lib_path=None, options=None, edits=None, inputs=None):
    """inputs: what `full_backward_inputs` returned for the same arguments, its oracle not yet differentiated (a caller that has
    looked at the oracle's outputs first)."""
    F, obs, P, noise, ref, orc = inputs or full_backward_inputs(K, N, T, B, hw, seed, flags, edits)
    core = SqairCore(F, hw, lib_path=lib_path, options=options)
    core.set_params(P)
    names = ["log_weights_per_timestep", "discrete_log_prob", "presence", "prop_pres", "disc_pres"]
    m = Model(obs, None, core, K, outputs=names)
    core.noise.copy_(torch.as_tensor(noise).reshape(core.noise.shape))
    core.forward(train=True)
    torch.cuda.synchronize()
    _same_decisions("prop_pres", core.out["prop_pres"].cpu().numpy(), ref.prop_pres.detach().numpy())
    _same_decisions("disc_pres", core.out["disc_pres"].cpu().numpy(), ref.disc_pres.detach().numpy())
    if not getattr(ref, "differentiated", False):
        orc.make_target(ref).backward()
        ref.differentiated = True
    core.backward()
    torch.cuda.synchronize()
    if options and options.get("slot_chain"):
        core.check_chain(train=True)   # (every launch of the in-launch slot chain completed: otherwise the tape means nothing)
    got = {k: v.cpu().numpy() for k, v in core.grads_by_name().items()}
    report = []
    for name, g in got.items():
        want = orc.P[name].grad
        want = np.zeros_like(g) if want is None else want.numpy().reshape(g.shape)
        err = float(np.abs(g - want).max())
        scale = float(np.abs(want).max())
        report.append((name, err, scale))
    return report, ref, core


# Gradient bar: 5e-4 of the parameter's largest gradient (measured: <= ~1e-4 in the regular regime).  The parameters below get
# 3e-3: `*.transform.scale_offset` is ONE scalar added to the four raw scales of every where posterior, so its gradient is the
# sum over all rows, frames, slots and the 4 scale columns of the gradient of `*.transform.l2.b` -- terms of both signs of size
# ~50 that cancel to ~0.3 (measured below: |grad| 0.29 against 49 for l2.b), which amplifies the fp32 rounding of the
# individual terms (each good to ~1e-4) by two orders of magnitude relative to the result.  Everything else holds the tight bar.
TIGHT, LOOSE = 5e-4, 3e-3
ILL_CONDITIONED = ("disc.transform.scale_offset", "prop.transform.scale_offset")


def check_report(report, tol=TIGHT, loose=ILL_CONDITIONED, ill_scale=False):
    gmax = max(s for _, _, s in report)
    if ill_scale:
        # `*.transform.scale_offset` is the SUM of the four scale columns of `*.transform.l2.b`'s gradient: judge its error on the
        # size of the terms it is made of (the loose bar above assumes the ~170x cancellation of the shipped sizes; other sizes
        # cancel harder)
        by = {n: s for n, _, s in report}
        report = [(n, e, max(s, by[n.replace("scale_offset", "l2.b")]) if n in loose else s) for n, e, s in report]
        loose = ()
    rel = lambda e, s: e / max(s, 1e-4 * gmax)
    bad = [(n, e, s) for n, e, s in report if not np.isfinite(e) or rel(e, s) > (LOOSE if n in loose else tol)]
    for n, e, s in sorted(report, key=lambda r: -rel(r[1], r[2]))[:8]:
        print("%-34s err %.3e  |grad|max %.3e  rel %.2e %s" % (n, e, s, rel(e, s), "<-- BAD" if (n, e, s) in bad else ""))
    assert not bad, [(n, "%.2e" % rel(e, s)) for n, e, s in bad]
