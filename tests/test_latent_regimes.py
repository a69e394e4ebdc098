"""No GPU: the classifier of tests/latent_regimes.py on hand-written latents, and, for every case of tests/test_regime_paths.py
(one shared table, tests/latent_regimes.py), what that file relies on without being able to check it on the device:

  * `stable_noise` finds a decision-stable draw within MAX_DRAWS;
  * the fp64 oracle alone reaches the regime the case is named after (`require`);
  * the fp32 oracle makes the same presence and id decisions;
  * for every gradient case, the draw is kink-stable: no bilinear sample coordinate of the oracle closer to an integer than fp32
    resolves (there the derivative of the sampler jumps, and the fp64 oracle and a correct fp32 implementation may differentiate
    on different sides);
  * for the "tight" cases, the fp32 oracle is within a QUARTER of the bar the HIP path is held to -- on every output, the bounds and
    the gradients through `make_target`.  That is what justifies holding the kernels to the unchanged bars in those regimes: a
    correct fp32 implementation has a factor of four to spare.  The "measured" cases (ill conditioned in fp32 whatever the
    implementation) are shown to be exactly that: their fp32 distance is printed, and the GPU file measures it again as its bar.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd.flags import make_flags
from tests import latent_regimes as LR

QUARTER = 0.25


# ---- the classifier on hand-written latents -----------------------------------------------------------------------------------------
CFG = SimpleNamespace(H=50, W=50, G=20, N=2)
LOGIT = lambda p: float(np.log(p) - np.log1p(-p))
MID = LOGIT(0.5)


def _outputs(where, where_scale=0.3, what_scale=0.3, presence=(1, 0), prop_logit=(0.0, 0.0), disc_logit=(0.0, 0.0), prev=(0, 0),
             disc_pres=(0, 0), canvas_max=0.5):
    """One (frame, row) cell with two slots; slot 1 absent unless said otherwise."""
    a = lambda v, w: np.broadcast_to(np.asarray(v, np.float64), (1, 1, 2, w) if w else (1, 1, 2)).copy()
    canvas = np.zeros((1, 1, 50, 50))
    canvas[0, 0, 3, 4] = canvas_max
    return {"where": np.asarray(where, np.float64).reshape(1, 1, 2, 4), "where_scale": a(where_scale, 4), "what_scale": a(what_scale, 5),
            "presence": a(presence, 0), "_prop_presence_logit": a(prop_logit, 0), "_disc_presence_logit": a(disc_logit, 0),
            "_prop_prev_presence": a(prev, 0), "disc_pres": a(disc_pres, 0), "canvas": canvas}


def _names(o, cfg=CFG):
    return {k for k, v in LR.classify(o, cfg).items() if v.any()}


def _where(sx, sy, tx, ty):
    return [LOGIT(sx), LOGIT(sy), float(np.arctanh(tx)), float(np.arctanh(ty))]


CENTRED = _where(0.5, 0.5, 0.0, 0.0)      # pitch 0.5 * 49 / 19 = 1.29, inside the frame
ABSENT = _where(0.99, 0.99, 0.9, 0.9)     # would be off the frame, minified, ... but its slot is absent


@pytest.mark.parametrize("where,want", [
    (CENTRED, set()),
    # the outermost sample point at 0.5 + 0.8 > 1 in x: 6 of 20 columns outside (0.3 of the points: not "mostly")
    (_where(0.5, 0.5, 0.8, 0.0), {"off_frame"}),
    # ... and in y too: 1 - 0.7 * 0.7 = 0.51 of the points outside
    (_where(0.5, 0.5, 0.8, -0.8), {"off_frame", "mostly_off"}),
    # pitch 0.1 * 49 / 19 = 0.26 in x
    (_where(0.1, 0.5, 0.0, 0.0), {"magnified"}),
    # pitch 0.9 * 49 / 19 = 2.3 in y, inside the frame
    (_where(0.5, 0.9, 0.0, 0.05), {"minified"}),
    # tiny, above the clamp
    (_where(0.01, 0.5, 0.0, 0.0), {"magnified", "tiny_scale"}),
    # below the clamp: sc = 1e-4 (not "tiny", which starts above the clamp)
    ([-11.0, 0.0, 0.0, 0.0], {"magnified", "scale_clamped"}),
    ([-11.0, LOGIT(0.02), 0.0, 0.0], {"magnified", "scale_clamped", "tiny_scale"}),
])
def test_geometry_patterns_on_and_off(where, want):
    assert _names(_outputs([where, ABSENT])) == want


def test_values_exactly_on_the_thresholds():
    """Every threshold is strict where the definition says "<" / ">" and inclusive where it says "at least"."""
    cfg = SimpleNamespace(H=39, W=39, G=20, N=2)            # pitch = 2 sc exactly (38 / 19)
    on = lambda **kw: _names(_outputs([kw.pop("where", CENTRED), ABSENT], **kw), kw.pop("cfg", CFG))
    # off_frame: sc + |tr| > 1, strictly (0.5 + 0.5 is the frame's edge: inside)
    w = [0.0, 0.0, float(np.arctanh(0.5)), 0.0]
    sc, tr = 0.5 * (1 + np.tanh(0.0)), np.tanh(w[2])
    assert (sc + abs(tr) > 1.0) == ("off_frame" in _names(_outputs([w, ABSENT])))
    # pitch exactly 0.5 (sc = 0.25) and exactly 2 (sc = 1 is out of a sigmoid's reach: use H = 77, pitch 4 sc, sc = 0.5)
    o = _outputs([[LOGIT(0.25), 0.0, 0.0, 0.0], ABSENT])
    pitch = 0.5 * (1 + np.tanh(0.5 * o["where"][0, 0, 0, 0])) * 2.0
    assert ("magnified" in _names(o, cfg)) == (pitch < 0.5)
    assert "magnified" in _names(_outputs([[LOGIT(0.2499), 0.0, 0.0, 0.0], ABSENT]), cfg)
    assert "magnified" not in _names(_outputs([[LOGIT(0.2501), 0.0, 0.0, 0.0], ABSENT]), cfg)
    cfg4 = SimpleNamespace(H=77, W=77, G=20, N=2)           # pitch = 4 sc
    assert "minified" not in _names(_outputs([[0.0, 0.0, 0.0, 0.0], ABSENT]), cfg4)        # sc = 0.5 exactly: pitch 2, not above
    assert "minified" in _names(_outputs([[LOGIT(0.5001), 0.0, 0.0, 0.0], ABSENT]), cfg4)
    # mostly_off: exactly a third counts (G = 3: one column of three outside)
    cfg3 = SimpleNamespace(H=50, W=50, G=3, N=2)
    assert "mostly_off" in _names(_outputs([_where(0.5, 0.5, 0.6, 0.0), ABSENT]), cfg3)    # points at 0.1, 0.6, 1.1 -> 1 / 3 outside
    assert "mostly_off" not in _names(_outputs([_where(0.5, 0.5, 0.4, 0.0), ABSENT]), cfg3)
    # the scales: strictly below
    assert "where_std_floor" not in on(where_scale=0.0101) and "where_std_floor" in on(where_scale=0.01009)
    assert "what_std_small" not in on(what_scale=0.01) and "what_std_small" in on(what_scale=0.00999)
    # the logit: at least 17, either sign, and only a live Bernoulli
    assert "saturated_logit" in on(prev=(1, 0), prop_logit=(17.0, 0.0)) and "saturated_logit" in on(prev=(1, 0), prop_logit=(-17.0, 0.0))
    assert "saturated_logit" not in on(prev=(1, 0), prop_logit=(16.999, 0.0))
    # the canvas: strictly above 1.5
    assert "bright_canvas" not in on(canvas_max=1.5) and "bright_canvas" in on(canvas_max=1.5001)


def test_absent_slots_and_dead_bernoullis_are_ignored():
    # slot 1 carries every extreme and is absent; slot 0 is centred
    o = _outputs([CENTRED, [-11.0, LOGIT(0.99), 3.0, 3.0]], where_scale=[[0.3] * 4, [0.01] * 4], what_scale=[[0.3] * 5, [0.001] * 5])
    assert _names(o) == set()
    o["presence"][...] = 1.0
    assert {"off_frame", "mostly_off", "magnified", "minified", "scale_clamped", "where_std_floor", "what_std_small"} <= _names(o)
    # propagation: live only where the object was present at t - 1; discovery: slot 0 always, slot j if slot j - 1 was found
    assert "saturated_logit" not in _names(_outputs([CENTRED, ABSENT], prev=(0, 0), prop_logit=(30.0, 30.0), disc_logit=(0.0, 30.0)))
    c = LR.classify(_outputs([CENTRED, ABSENT], prev=(0, 1), prop_logit=(30.0, 30.0), disc_logit=(-20.0, 30.0), disc_pres=(0, 0)), CFG)
    assert c["saturated_logit"][0, 0].tolist() == [[False, True], [True, False]]
    c = LR.classify(_outputs([CENTRED, ABSENT], disc_logit=(0.0, 30.0), disc_pres=(1, 0)), CFG)
    assert c["saturated_logit"][0, 0].tolist() == [[False, False], [False, True]]


def test_logits_are_recovered_from_the_oracles_probabilities():
    """The oracle writes the pre-merge PROBABILITIES; fp64 keeps a logit of 25 apart from one of 17, and p = 1 counts."""
    o = _outputs([CENTRED, ABSENT], prev=(1, 1))
    del o["_prop_presence_logit"], o["_disc_presence_logit"]
    sig = lambda x: 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))
    o["_disc_presence_prob"] = sig([0.0, 0.0]).reshape(1, 1, 2)
    o["_prop_presence_prob"] = sig([25.0, 16.9]).reshape(1, 1, 2)
    assert LR.classify(o, CFG)["saturated_logit"][0, 0, 0].tolist() == [True, False]
    o["_prop_presence_prob"] = np.array([1.0, 0.0]).reshape(1, 1, 2)
    assert LR.classify(o, CFG)["saturated_logit"][0, 0, 0].tolist() == [True, True]


def test_overlap_needs_two_present_objects_on_one_pixel():
    two = [CENTRED, CENTRED]
    assert "overlap" in _names(_outputs(two, presence=(1, 1)))
    assert "overlap" not in _names(_outputs(two, presence=(1, 0)))
    apart = [_where(0.3, 0.3, -0.5, -0.5), _where(0.3, 0.3, 0.5, 0.5)]
    assert "overlap" not in _names(_outputs(apart, presence=(1, 1)))


def test_counts_table_and_require():
    o = _outputs([_where(0.5, 0.5, 0.8, -0.8), ABSENT], canvas_max=2.0)
    c = LR.counts_of(o, CFG)
    assert c["cells"] == 2 and c["rows"] == 1 and c["off_frame"] == 1 and c["mostly_off"] == 1 and c["bright_canvas"] == 1
    assert LR.require(c, off_frame=1, bright_canvas=1) is c
    with pytest.raises(AssertionError) as e:
        LR.require(c, off_frame=1, minified=1, overlap=2)
    msg = str(e.value)
    assert "'minified': (0, 1)" in msg and "'overlap': (0, 2)" in msg and "'off_frame'" not in msg.split(";")[0]
    assert all("{}=".format(k) in msg for k in LR.PATTERNS)
    with pytest.raises(AssertionError, match="unknown pattern"):
        LR.require(c, offframe=1)
    with pytest.raises(AssertionError, match="unknown pattern"):
        LR.require_prior(dict(prior_where_std_floor=1), where_std_floor=1)


def test_edits_are_pure_named_and_tagged():
    F = make_flags(k_particles=2, n_steps_per_image=2)
    P = LR.edited_params(F, (50, 50), 3, 0.05)
    keep = {k: v.copy() for k, v in P.items()}
    for name, (fn, purpose, tag) in LR.EDITS.items():
        Q = fn(P, F)
        assert all(np.array_equal(P[k], keep[k]) for k in P), name               # the input is left alone
        changed = [k for k in P if not np.array_equal(Q[k], P[k])]
        assert changed and len(changed) <= 4, (name, changed)                    # a few heads, never the whole model
        assert all(Q[k].dtype == np.float32 for k in Q) and purpose and tag in ("tight", "measured")
    assert {n for n, e in LR.EDITS.items() if e[2] == "measured"} == {"where_spread", "tiny_scale"}
    both = LR.edited_params(F, (50, 50), 3, 0.05, edits=("std_floor", "bright_decoder"))
    assert float(both["dec.l2.b"][0]) == 1.5 and float(both["disc.transform.scale_offset"]) == -12.0
    assert LR.conditioning(("std_floor", "tiny_scale")) == "measured" and LR.conditioning(LR.COMBINED) == "tight"


def test_every_pattern_is_required_by_a_forward_and_a_backward_case():
    fwd = set().union(*(set(c[7]) for c in LR.FORWARD.values()))
    bwd = set().union(*(set(c[8]) for c in LR.BACKWARD.values()))
    assert fwd == set(LR.PATTERNS) and bwd == set(LR.PATTERNS), (set(LR.PATTERNS) - fwd, set(LR.PATTERNS) - bwd)
    for table, at in ((LR.FORWARD, 6), (LR.BACKWARD, 7)):
        assert any("floored_prior" in c[at] for c in table.values())
        assert set(LR.SINGLE) <= set(table) and "combined" in table


# ---- the cases of tests/test_regime_paths.py, on the oracle alone ---------------------------------------------------------------------
def _show(case, what, dist, bar):
    worst = max(dist, key=dist.get)
    print("{}: {} fp32 oracle - fp64 oracle {:.2e} ({}), a quarter of the bar {:.2e}".format(case, what, dist[worst], worst, QUARTER * bar))
    return dist[worst]


@functools.lru_cache(maxsize=None)
def _forward(case):
    from tests.hip_util import run_oracle
    from tests.pass_cases import live_oracle_inputs
    K, N, T, B, hw, flags, edits, need = LR.FORWARD[case]
    F = make_flags(k_particles=K, n_steps_per_image=N, **flags)
    x = live_oracle_inputs(F, hw, T, B, edits=edits)      # (fails if no decision-stable draw within MAX_DRAWS)
    r32 = run_oracle(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"], dtype=torch.float32)
    return F, x, r32


@pytest.mark.parametrize("case", sorted(LR.FORWARD))
def test_forward_case_reaches_its_regime_and_is_conditioned(case):
    K, N, T, B, hw, flags, edits, need = LR.FORWARD[case]
    F, x, r32 = _forward(case)
    cfg = O.make_cfg(F, hw)
    counts = LR.counts_of(x["ref"].outputs, cfg)
    print(LR.table(counts))
    LR.require(counts, **need)
    if "floored_prior" in edits:
        LR.require_prior(LR.prior_counts(x["P"], cfg, x["obs"], x["noise"], x["d"]["nums"]), **LR.PRIOR_REACH)
    assert LR.same_decisions(r32, x["ref"]), "the fp32 oracle decides differently: the draw is not decision-stable in fp32"
    out = _show(case, "outputs", LR.output_distances(r32, x["ref"]), LR.OUTPUT_BAR)
    bound = _show(case, "bounds", LR.bound_distances(r32, x["ref"]), LR.BOUND_BAR)
    if LR.conditioning(edits) == "tight":
        assert out <= QUARTER * LR.OUTPUT_BAR and bound <= QUARTER * LR.BOUND_BAR


@functools.lru_cache(maxsize=None)
def _backward(edits, flags_items):
    from tests.pass_cases import full_backward_inputs
    F, obs, P, noise, ref, orc = full_backward_inputs(3, 3, 3, 3, LR.BWD_HW, LR.BWD_SEED, dict(flags_items), edits,
                                                       seed0=LR.bwd_noise_seed0(edits))
    orc.make_target(ref).backward()
    o32 = O.SqairOracle(P, O.make_cfg(F, LR.BWD_HW), torch.float32, requires_grad=True)
    r32 = o32.model(obs, noise)
    o32.make_target(r32).backward()
    cfg = O.make_cfg(F, LR.BWD_HW)
    ref.kinks = LR.kink_clearance(P, cfg, obs, noise)
    ref.prior = LR.prior_counts(P, cfg, obs, noise) if "floored_prior" in edits else None
    return F, obs, P, noise, ref, orc, r32, o32


@pytest.mark.parametrize("case", sorted(LR.BACKWARD))
def test_backward_case_reaches_its_regime_and_is_conditioned(case):
    K, N, T, B, flags, options, wide, edits, need = LR.BACKWARD[case]
    assert (K, N, T, B) == (3, 3, 3, 3)
    F, obs, P, noise, ref, orc, r32, o32 = _backward(edits, tuple(sorted(flags.items())))
    cfg = O.make_cfg(F, LR.BWD_HW)
    counts = LR.counts_of(ref.outputs, cfg)
    print(LR.table(counts))
    LR.require(counts, **need)
    if "floored_prior" in edits:
        LR.require_prior(ref.prior, **LR.PRIOR_REACH)
    assert LR.same_decisions(r32, ref)
    # a gradient case needs a kink-stable draw too (tests/latent_regimes.py: KINK_ULPS): no bilinear sample coordinate closer to an
    # integer than fp32 resolves, where the fp64 oracle's one-sided derivative and an fp32 implementation's may differ
    kinks = ref.kinks
    print(case + ":", kinks.closest())
    assert kinks.clearance >= 1.0, kinks.closest() + ": choose another noise seed (latent_regimes.BWD_NOISE_SEED0)"
    out = _show(case, "outputs", LR.output_distances(r32, ref), LR.OUTPUT_BAR)
    bound = _show(case, "bounds", LR.bound_distances(r32, ref), LR.BOUND_BAR)
    rel = LR.gradient_rel(LR.gradient_report(LR.oracle_grads(o32), LR.oracle_grads(orc)))
    tight = {n: v for n, v in rel.items() if n not in LR.GRAD_LOOSE_NAMES}
    loose = {n: v for n, v in rel.items() if n in LR.GRAD_LOOSE_NAMES}
    gt, gl = _show(case, "gradients", tight, LR.GRAD_TIGHT), _show(case, "scale_offset gradients", loose, LR.GRAD_LOOSE)
    if LR.conditioning(edits) == "tight":
        assert out <= QUARTER * LR.OUTPUT_BAR and bound <= QUARTER * LR.BOUND_BAR
        assert gt <= QUARTER * LR.GRAD_TIGHT and gl <= QUARTER * LR.GRAD_LOOSE
    else:
        # ill conditioned in fp32 whatever the implementation: the fp32 ORACLE itself is beyond a quarter of the tight bar somewhere
        assert max(gt / LR.GRAD_TIGHT, out / LR.OUTPUT_BAR) > QUARTER, "well conditioned after all: tag the edit \"tight\""


def test_the_clamps_own_gradient_path_is_zero_at_the_bars_resolution(monkeypatch):
    """The reference clips the glimpse scale with `clip_preserve` (ops.py:33-42): forward max(s, 1e-4), gradient of the identity.
    Below the clamp that path carries sigmoid'(l) ~ 2e-5 times d target / d sc into `disc.transform.l2.b[:2]`.  Measured here on the
    oracle alone, by differentiating once with the reference's clip and once with a plain clamp (whose gradient below 1e-4 is
    exactly zero): the two entries differ by ~1e-4 against a bar of ~0.04 on that parameter.  So the clamp case of
    tests/test_regime_paths.py does not depend on how the clip is differentiated -- the clamp's contribution is zero at the bar's
    resolution -- and what it pins is that the 1 / sc = 1e4 of the inverse transformer's grid does not blow the adjoints up."""
    edits = LR.BACKWARD["scale_clamp"][7]
    F, obs, P, noise, ref, orc, _, _ = _backward(edits, ())
    assert LR.counts_of(ref.outputs, O.make_cfg(F, LR.BWD_HW))["scale_clamped"] >= 4
    want = LR.oracle_grads(orc)["disc.transform.l2.b"]
    monkeypatch.setattr(O, "clip_preserve_min", lambda x, lo: torch.clamp(x, min=lo))
    hard = O.SqairOracle(P, O.make_cfg(F, LR.BWD_HW), torch.float64, requires_grad=True)
    m = hard.model(obs, noise)
    assert LR.same_decisions(m, ref)
    hard.make_target(m).backward()
    got = LR.oracle_grads(hard)["disc.transform.l2.b"]
    bar = LR.GRAD_TIGHT * np.abs(want).max()
    print("d target / d disc.transform.l2.b[:2]: clip_preserve", want[:2], "plain clamp", got[:2], "bar", bar)
    assert (np.abs(got[:2] - want[:2]) <= LR.CLAMP_CONTRIBUTION * bar).all()
    assert (np.abs(want[:2]) >= 100.0 * bar).all(), "the two entries must carry a gradient worth comparing"


def test_stream_case_reaches_its_regime_and_is_conditioned():
    from tests.hip_util import run_oracle
    from tests.pass_cases import live_oracle_inputs
    c = LR.STREAM
    F = make_flags(k_particles=c["K"], n_steps_per_image=c["N"])
    x = live_oracle_inputs(F, c["hw"], c["T"], c["B"], edits=c["edits"])
    counts = LR.counts_of(x["ref"].outputs, O.make_cfg(F, c["hw"]))
    print(LR.table(counts))
    LR.require(counts, **c["minimums"])
    assert all(sum(sizes) == c["T"] for sizes in c["chunks"])
    r32 = run_oracle(F, c["hw"], x["P"], x["obs"], x["noise"], nums=x["d"]["nums"], dtype=torch.float32)
    assert LR.same_decisions(r32, x["ref"])
    assert _show("stream", "outputs", LR.output_distances(r32, x["ref"]), LR.OUTPUT_BAR) <= QUARTER * LR.OUTPUT_BAR
    assert _show("stream", "bounds", LR.bound_distances(r32, x["ref"]), LR.BOUND_BAR) <= QUARTER * LR.BOUND_BAR


def test_stream_training_case_reaches_its_regime_and_is_conditioned():
    """The oracle side of `chunk_two_case` (tests/stream_cases.py, the case of tests/test_stream_train.py) without SMC: the same frames, the same generator, so the
    same two noise draws; chunk 2 from the carried state with the last lane reset."""
    from tests import tbptt_ref as TR
    from tests.stream_cases import ORACLE_HW as HW, stable_chunk as _stable
    from tests.stream_harness import train_setup
    c = LR.STREAM_TRAIN
    B, T = 3, 3
    F, obs, P = train_setup(c["flags"], B, 2 * T, HW, 23, edits=c["edits"])
    K = int(F.k_particles)
    R = B * K
    cfg = O.make_cfg(F, HW)
    orc = O.SqairOracle(P, cfg, torch.float64, requires_grad=True)
    rng = np.random.default_rng(11)
    with LR.kink_recorder() as kinks:    # (both chunks, rejected draws included: what the GPU leg's `require` hook sees)
        noise1, _, out1, st1 = _stable(orc, obs[:T], K, None, rng, F, R, T, grad=False)
        src = np.arange(R)
        src[(B - 1) * K:] = -1
        noise2, target, out2, _ = _stable(orc, obs[T:], K, orc.gather_state(st1, src), rng, F, R, T, grad=True)
    print("stream training:", kinks.closest())
    assert kinks.clearance >= 1.0, kinks.closest()
    counts = LR.counts_of(out2, cfg)
    print(LR.table(counts))
    LR.require(counts, **c["minimums"])
    target.backward()
    o32 = O.SqairOracle(P, cfg, torch.float32, requires_grad=True)
    with torch.no_grad():
        _, o1, s1 = TR.chunk_target(o32, obs[:T], noise1, K, None)
    t32, o2, _ = TR.chunk_target(o32, obs[T:], noise2, K, o32.gather_state(s1, src))
    for k in ("presence", "obj_id"):
        assert np.array_equal(o1[k].numpy(), out1[k].numpy()) and np.array_equal(o2[k].detach().numpy(), out2[k].detach().numpy()), k
    t32.backward()
    rel = LR.gradient_rel(LR.gradient_report(LR.oracle_grads(o32), LR.oracle_grads(orc)))
    tight = {n: v for n, v in rel.items() if n not in LR.GRAD_LOOSE_NAMES}
    loose = {n: v for n, v in rel.items() if n in LR.GRAD_LOOSE_NAMES}
    assert _show("stream training", "gradients", tight, LR.GRAD_TIGHT) <= QUARTER * LR.GRAD_TIGHT
    assert _show("stream training", "scale_offset gradients", loose, LR.GRAD_LOOSE) <= QUARTER * LR.GRAD_LOOSE


def test_particle_filter_case_reaches_saturated_logits_at_every_step():
    """The fp64 filter of tests/smc_ref.py on its OWN ancestors (the GPU test gathers through the device's, which agree wherever
    the weights are not ambiguous): every step's proposal holds live Bernoullis with |logit| >= 17, and a decision-stable draw
    exists at every step."""
    from sqair_amd.data import make_sequences, to_float
    from tests import smc_ref as S
    from tests.hip_util import MARGIN, draw_noise, params32, presence_margins
    from tests.stream_cases import DRAWS, ORACLE_HW as HW
    c = LR.SMC
    F = make_flags(**c["flags"])
    B, TS, K, N = c["B"], c["frames_per_step"], int(F.k_particles), int(F.n_steps_per_image)
    obs = to_float(make_sequences(B, T=c["frames"], canvas=HW, seed=19)["imgs"])
    P = LR.apply_edits(params32(F, HW, 3, 0.05, obs.mean((0, 1))), F, c["edits"])
    pf = S.ParticleFilter(P, F, HW, B)
    cfg = O.make_cfg(F, HW)
    rng = np.random.default_rng(7)
    went = 0
    for s in range(c["frames"] // TS):
        fr = obs[s * TS:(s + 1) * TS]
        for attempt in range(DRAWS):
            noise = draw_noise(rng, TS, B * K, N, 4 + int(F.n_what) + 1)
            prop = pf.propose(fr, noise)
            if float(presence_margins(prop[0], noise).min()) >= MARGIN:
                break
        else:
            raise AssertionError("no decision-stable noise draw at step {}".format(s))
        LR.require(LR.counts_of(prop[0], cfg), **c["minimums"])
        lw0, lz0 = pf.log_w.copy(), pf.log_z.copy()
        ref, rw = pf.commit(prop)
        u = S.smc_uniform(np.arange(B), pf.state.t.numpy()[::K], 41)
        r = S.resample(lw0, ref["log_weights_per_timestep"].numpy(), lz0, u, K, c["ess_frac"])
        went += int(r.go.sum())
        pf.advance(r.src, r.go)
    assert went > 0, "the case must resample"


def test_forecast_case_reaches_the_floored_prior():
    """The forecast reference on its own sampled latents: with `floored_prior` every prior of a present object has both scales at
    the floor and a saturated presence logit, and the rollout stays decision-stable."""
    from tests.hip_util import params32
    from tests.stream_cases import reference_rollout as _reference_rollout
    from tests.stream_harness import frames as _frames
    c = LR.FORECAST
    F = make_flags(**c["flags"])
    obs = _frames(c["hw"], c["B"], c["S"], 19)
    P = LR.apply_edits(params32(F, c["hw"], 3, 0.05, obs.mean((0, 1))), F, c["edits"])
    noise, fnoise, ref, state, mg = _reference_rollout(F, P, obs, c["hw"], c["B"], c["S"], c["Fn"])
    counts = LR.forecast_prior_counts(ref)
    print(counts, "present objects per frame", ref["presence"].sum((1, 2)).tolist())
    LR.require_prior(counts, **c["minimums"])
    assert float(ref["presence"][-1].sum()) >= 4, "objects must survive to the last forecast frame"
