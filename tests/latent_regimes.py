"""Which LATENT VALUES a test case reaches: a classifier of the ORACLE's latents, coverage gates on its counts, and the parameter
edits that move the oracle there.

Every parity case of the other suites runs at `params32(F, hw, seed, 0.02 ... 0.05)`: freshly initialised weights.  There the glimpse
scales sit in 0.33 ... 0.71, the posterior scales well above their floors, the presence logits below 6 and the canvas below 0.75.  A
trained (or diverging) model visits magnified and minified glimpses, glimpses that hang off the frame, the 1e-4 clamp of the scale,
floored standard deviations, Bernoullis whose fp32 sigmoid is exactly 1 and canvases above 2.  `EDITS` moves a few heads of the
initialised parameters so that the oracle visits those values while the problem stays well conditioned; `classify` names the regimes
per cell, `count` sums them, `require` fails with the whole table when a minimum is missed.  The inputs are oracle outputs only,
never anything the HIP path computed (the same design as tests/presence_patterns.py).

`FORWARD`, `BACKWARD`, `STREAM`, `STREAM_TRAIN`, `SMC` and `FORECAST` are the one table of the cases of tests/test_regime_paths.py
(-m gpu); tests/test_latent_regimes.py proves on the CPU, for every one of them, that the oracle alone reaches the regime, that the
noise draw is decision-stable (and, for gradients, kink-stable: `kink_recorder`), and (for the "tight" ones) that the fp32 oracle
sits within a quarter of the bar the HIP path is held to.
"""
import numpy as np
import torch

from oracle import sqair_oracle as O
from sqair_amd.params import init_params

CELL_PATTERNS = ("off_frame", "mostly_off", "magnified", "minified", "scale_clamped", "tiny_scale", "where_std_floor",
                 "what_std_small", "saturated_logit")
ROW_PATTERNS = ("bright_canvas", "overlap")
PATTERNS = CELL_PATTERNS + ROW_PATTERNS

SCALE_CLAMP = 1e-4          # modules.py:205-206: sx, sy >= 1e-4
TINY_SCALE = 0.03
WHERE_STD_FLOOR = 0.0101    # softplus(.) + 1e-2
WHAT_STD_SMALL = 0.01
SATURATED = 17.0            # the fp32 sigmoid rounds to exactly 1 from about here
BRIGHT = 1.5
OVERLAP = 1.5               # sigmoid(-10 + 20 nz): two objects on one pixel


def _np(x):
    return np.asarray(x.detach().numpy() if hasattr(x, "detach") else x, dtype=np.float64)


def _sigmoid(x):
    return 0.5 * (1.0 + np.tanh(0.5 * x))


def _logit(p):
    with np.errstate(divide="ignore"):
        return np.log(p) - np.log1p(-p)


def classify(outputs, cfg):
    """outputs: an oracle output dictionary (Model.outputs of oracle/sqair_oracle.py, or hand-written arrays under the same
    names); cfg: anything with H, W, G, N.  With sc = max(sigmoid(where[..., :2]), 1e-4) and tr = tanh(where[..., 2:]), returns
    {pattern: bool array}.  Over (frame, row, slot) cells, true only where the slot is PRESENT (the last pattern: where its
    Bernoulli is live), [T, R, N]:

      off_frame         sc + |tr| > 1 in x or y: the glimpse's outermost sample point lies outside the frame
      mostly_off        at least a third of the G x G sample points lie outside the frame
      magnified         the sample pitch sc (L - 1) / (G - 1) in frame pixels is below 0.5 in x or y (L = W, H)
      minified          that pitch is above 2 in x or y
      scale_clamped     sigmoid(where) < 1e-4 in x or y: the clamp is active
      tiny_scale        1e-4 < sc < 0.03 in x or y
      where_std_floor   some where_scale < 0.0101 (the softplus + 1e-2 floor)
      what_std_small    some what_scale < 0.01
      saturated_logit   a LIVE Bernoulli with |logit| >= 17; "live" as tests/hip_util.presence_margins has it: a propagation slot
                        whose object was present at t - 1, a discovery slot whose predecessor was found (or slot 0); [T, R, 2, N]

    and over (frame, row) cells, [T, R]:

      bright_canvas     max of the canvas above 1.5
      overlap           some pixel with sum_slots presence * st_insert(ones) >= 1.5: two objects saturate the blend"""
    N, G, H, W = int(cfg.N), int(cfg.G), int(cfg.H), int(cfg.W)
    where = _np(outputs["where"])
    T, R = where.shape[:2]
    where = where.reshape(T, R, N, 4)
    pres = _np(outputs["presence"]).reshape(T, R, N) > 0.5
    sg = _sigmoid(where[..., :2])
    sc = np.maximum(sg, SCALE_CLAMP)
    tr = np.tanh(where[..., 2:])
    g = np.linspace(-1.0, 1.0, G)
    pos = sc[..., None] * g + tr[..., None]                                   # [T, R, N, 2 (x, y), G] in [-1, 1] frame units
    inside = (np.abs(pos) <= 1.0).sum(-1) / float(G)                          # fraction of the columns / rows inside
    pitch = sc * (np.array([W, H], dtype=np.float64) - 1.0) / max(G - 1, 1)
    out = dict(
        off_frame=(sc + np.abs(tr) > 1.0).any(-1),
        mostly_off=(1.0 - inside[..., 0] * inside[..., 1]) >= 1.0 / 3.0,
        magnified=(pitch < 0.5).any(-1),
        minified=(pitch > 2.0).any(-1),
        scale_clamped=(sg < SCALE_CLAMP).any(-1),
        tiny_scale=((sc > SCALE_CLAMP) & (sc < TINY_SCALE)).any(-1),
        where_std_floor=(_np(outputs["where_scale"]).reshape(T, R, N, 4) < WHERE_STD_FLOOR).any(-1),
        what_std_small=(_np(outputs["what_scale"]).reshape(T, R, N, -1) < WHAT_STD_SMALL).any(-1),
    )
    out = {k: v & pres for k, v in out.items()}
    # live Bernoullis: exactly the set presence_margins measures
    def logits(kind):
        if "_{}_presence_logit".format(kind) in outputs:
            return _np(outputs["_{}_presence_logit".format(kind)]).reshape(T, R, N)
        return _logit(_np(outputs["_{}_presence_prob".format(kind)]).reshape(T, R, N))
    live = np.zeros((T, R, 2, N), bool)
    live[:, :, 0] = _np(outputs["_prop_prev_presence"]).reshape(T, R, -1)[..., :N] > 0.5
    dp = _np(outputs["disc_pres"]).reshape(T, R, N)
    live[:, :, 1] = np.concatenate([np.ones_like(dp[..., :1]), dp[..., :-1]], -1) > 0.5
    lg = np.stack([logits("prop"), logits("disc")], 2)
    out["saturated_logit"] = live & (np.abs(lg) >= SATURATED)
    out["bright_canvas"] = _np(outputs["canvas"]).reshape(T, R, -1).max(-1) > BRIGHT
    ones = torch.ones(T * R * N, G, G, dtype=torch.float64)
    nz = O.st_insert(ones, torch.as_tensor(where.reshape(-1, 4)), H, W).numpy().reshape(T, R, N, H, W)
    out["overlap"] = (nz * pres[..., None, None]).sum(2).max((2, 3)) >= OVERLAP
    assert tuple(out) == PATTERNS
    return out


def count(patterns):
    c = {k: int(v.sum()) for k, v in patterns.items()}
    c["cells"] = int(patterns["off_frame"].size)
    c["rows"] = int(patterns["overlap"].size)
    return c


def table(counts):
    return "latent regimes over {} (frame, row, slot) and {} (frame, row) cells: ".format(counts["cells"], counts["rows"]) + " ".join(
        "{}={}".format(k, counts[k]) for k in PATTERNS)


def require(counts, **minimums):
    """Fails, with the whole table, when the case does not reach `pattern >= minimum` for every keyword."""
    unknown = [k for k in minimums if k not in PATTERNS]
    assert not unknown, "unknown pattern(s) {}".format(unknown)
    missed = {k: (counts[k], m) for k, m in minimums.items() if counts[k] < m}
    assert not missed, "the case does not reach the latent regimes it is meant to test: {} (have, need); {}".format(
        missed, table(counts))
    return counts


def counts_of(outputs, cfg):
    return count(classify(outputs, cfg))


# ----------------------------------------------------------------------------- the edits
EDITS = {}   # name -> (function(P, F) -> P, what it is for, "tight" | "measured")


def _edit(name, purpose, conditioning):
    assert conditioning in ("tight", "measured")

    def register(fn):
        def pure(P, F):
            Q = {k: np.array(v, copy=True) for k, v in P.items()}
            fn(Q, F)
            assert all(Q[k].dtype == P[k].dtype and Q[k].shape == np.shape(P[k]) for k in P)
            return Q
        EDITS[name] = (pure, purpose, conditioning)
        return pure
    return register


def _where_bias(P, values):
    P["disc.transform.l2.b"][:4] = np.asarray(values, P["disc.transform.l2.b"].dtype)


@_edit("magnify_off_frame", "discovery glimpses of scale 0.09 ... 0.46 shifted to the frame's edge: magnified crops with taps outside", "tight")
def _(P, F):
    _where_bias(P, [-1.5, -1.5, 1.2, -1.2])


@_edit("minify_off_frame", "discovery glimpses of scale 0.66 ... 0.94, shifted: minified crops, most sample points outside", "tight")
def _(P, F):
    _where_bias(P, [1.5, 1.5, 1.0, -1.0])


@_edit("scale_clamp", "every discovery scale below the 1e-4 clamp (straight-through gradient)", "tight")
def _(P, F):
    _where_bias(P, [-11.0, -11.0, 0.3, -0.3])


@_edit("std_floor", "where_scale at its softplus + 1e-2 floor, what_scale below 0.01", "tight")
def _(P, F):
    nw = int(F.n_what)
    for core in ("disc", "prop"):
        P[core + ".transform.scale_offset"][...] = -12.0
    for head in ("enc", "prop"):
        P[head + ".what_head.b"][nw:] = -10.0


@_edit("saturated_presence", "live presence logits beyond 17: the fp32 sigmoid is exactly 1", "tight")
def _(P, F):
    P["prop.steps.l1.b"][...] = 25.0
    P["disc.steps.l1.b"][...] = 18.0


@_edit("bright_decoder", "decoded glimpses near 1.5 before the sum: canvas above 2, a large negative ELBO", "tight")
def _(P, F):
    P["dec.l2.b"][...] = 1.5


@_edit("floored_prior", "propagation prior with floored scales and a saturated presence logit", "tight")
def _(P, F):
    nw = int(F.n_what)
    b = P["prop.prior_linear.b"]
    assert b.shape[-1] == 2 * (4 + nw) + 1
    b[0] = 20.0
    b[1 + 4 + nw:] = -12.0


@_edit("where_spread", "data-dependent spread of the where means (x 3 on the last transform layer's loc columns)", "measured")
def _(P, F):
    for core in ("disc", "prop"):
        P[core + ".transform.l2.w"][:, :4] *= 3.0


@_edit("tiny_scale", "discovery scales 0.001 ... 0.02, above the clamp: the regime of sq_sigmoid_geo", "measured")
def _(P, F):
    _where_bias(P, [-6.0, -6.0, 0.3, -0.3])


COMBINED = ("std_floor", "saturated_presence", "bright_decoder")


def conditioning(edits):
    """ "measured" if any edit of the list is, "tight" otherwise."""
    return "measured" if any(EDITS[e][2] == "measured" for e in edits) else "tight"


def apply_edits(P, F, edits):
    for e in edits or ():
        P = EDITS[e][0](P, F)
    return P


def edited_params(F, hw, seed, jitter, mean_img=None, edits=()):
    """`params32(F, hw, seed, jitter, mean_img)` of tests/hip_util.py with the named edits applied in order (float32)."""
    P = init_params(F, hw, seed=seed, mean_img=mean_img, jitter=jitter)
    return apply_edits({k: np.asarray(v, dtype=np.float32) for k, v in P.items()}, F, edits)


# ----------------------------------------------------------------------------- the cases (shared by the CPU and the GPU file)
# What each edit must reach, required from the oracle's outputs alone.  (Minimums well below what was measured on the CPU: a gate on
# "reaches the regime at all", not a fingerprint of one draw.)
REACH = {
    "magnify_off_frame": dict(off_frame=4, mostly_off=2, magnified=2),
    "minify_off_frame": dict(off_frame=4, mostly_off=2, minified=2),
    "scale_clamp": dict(scale_clamped=4),
    "std_floor": dict(where_std_floor=4, what_std_small=2),
    "saturated_presence": dict(saturated_logit=4),
    "bright_decoder": dict(bright_canvas=2, overlap=1),
    "floored_prior": {},      # (its reach is in the PRIOR's statistics: `prior_counts`, PRIOR_REACH)
    "where_spread": dict(off_frame=4),
    "tiny_scale": dict(tiny_scale=4, magnified=4),
}


def minimums(edits, without=()):
    """What a case with these edits must reach: the largest minimum any of its edits asks for per pattern.  without: patterns
    another edit of the same case takes away (a magnified glimpse inserts a small object: its canvas stays below 1.5)."""
    m = {}
    for e in edits:
        for k, v in REACH[e].items():
            m[k] = max(m.get(k, 0), v)
    return {k: v for k, v in m.items() if k not in without}


PRIOR_PATTERNS = ("prior_where_std_floor", "prior_what_std_floor", "prior_saturated_logit")


def prior_counts(P, cfg, obs, noise, nums=None):
    """The propagation PRIOR's statistics are no output of the oracle: this runs the fp64 oracle once more on the same inputs with
    `propagate_prior` recorded, and counts, over the (frame, row, slot) cells whose object was present at t - 1 (the others'
    prior terms are masked), the priors with a where scale / a what scale below 0.0101 and with |logit| >= 17."""
    orc = O.SqairOracle(P, cfg, torch.float64)
    seen, inner = [], orc.propagate_prior

    def recorded(z_tm1, prior_state):
        stats, state = inner(z_tm1, prior_state)
        seen.append((stats[1], stats[3], stats[4], z_tm1[2]))
        return stats, state
    orc.propagate_prior = recorded
    with torch.no_grad():
        orc.model(obs, noise, num=nums)
    return prior_counts_of(seen)


def prior_counts_of(seen):
    """seen: a list of (where_scale [R, N, 4], what_scale [R, N, nw], logit [R, N, 1], presence at t - 1 [R, N, 1]) per frame."""
    live = np.stack([_np(s[3])[..., 0] > 0.5 for s in seen])
    c = dict(prior_where_std_floor=int((live & np.stack([(_np(s[0]) < WHERE_STD_FLOOR).any(-1) for s in seen])).sum()),
             prior_what_std_floor=int((live & np.stack([(_np(s[1]) < WHERE_STD_FLOOR).any(-1) for s in seen])).sum()),
             prior_saturated_logit=int((live & np.stack([np.abs(_np(s[2])[..., 0]) >= SATURATED for s in seen])).sum()))
    c["prior_cells"] = int(live.sum())
    return c


def require_prior(counts, **minimums):
    unknown = [k for k in minimums if k not in PRIOR_PATTERNS]
    assert not unknown, "unknown pattern(s) {}".format(unknown)
    missed = {k: (counts[k], m) for k, m in minimums.items() if counts[k] < m}
    assert not missed, "the propagation prior does not reach the regime the case is meant to test: {} (have, need); {}".format(
        missed, counts)
    return counts


PRIOR_REACH = dict(prior_where_std_floor=4, prior_what_std_floor=4, prior_saturated_logit=4)   # of every case with `floored_prior`


SINGLE = ("magnify_off_frame", "minify_off_frame", "scale_clamp", "std_floor", "saturated_presence", "bright_decoder", "floored_prior",
          "where_spread", "tiny_scale")
LSTM3 = dict(transition="LSTM", time_transition="LSTM", prior_transition="LSTM")
NOT_BRIGHT = ("bright_canvas",)

# name: (K, N, T, B, frame, flags, edits, minimums).  The shipped shape (N = 4 slots, 50 x 50) takes the specialised kernels.
FORWARD = {e: (3, 4, 4, 4, (50, 50), {}, (e,), minimums((e,))) for e in SINGLE}
FORWARD.update({
    "combined": (3, 4, 4, 4, (50, 50), {}, COMBINED, minimums(COMBINED)),
    "combined_off_frame": (3, 4, 4, 4, (50, 50), {}, COMBINED + ("minify_off_frame",), minimums(COMBINED + ("minify_off_frame",))),
    "wide_n_what_64": (3, 3, 3, 3, (32, 40), dict(n_what=64), COMBINED + ("magnify_off_frame",),
                       minimums(COMBINED + ("magnify_off_frame",), NOT_BRIGHT)),
    # 130 columns: wider than a wavefront (the row-wave canvas kernels)
    "row_wave_40x130": (2, 3, 3, 3, (40, 130), {}, COMBINED + ("minify_off_frame",), minimums(COMBINED + ("minify_off_frame",))),
    # 65 000 pixels: above the crop's LDS staging limit (the unstaged gather); at this size a scale of 0.09 is a pitch above 1
    "unstaged_crop_250x260": (2, 3, 2, 2, (250, 260), {}, ("magnify_off_frame", "saturated_presence"),
                              dict(off_frame=4, saturated_logit=4)),
    "prior_rw": (3, 3, 4, 3, (50, 50), dict(prop_prior_type="rw"), ("saturated_presence", "floored_prior"),
                 minimums(("saturated_presence",))),
    "prior_guided": (3, 3, 4, 3, (50, 50), dict(prop_prior_type="guided", masked_glimpse=False), ("saturated_presence", "floored_prior"),
                     minimums(("saturated_presence",))),
    "no_rec_where_prior": (3, 3, 3, 3, (50, 50), dict(rec_where_prior=False), COMBINED + ("magnify_off_frame",),
                           minimums(COMBINED + ("magnify_off_frame",), NOT_BRIGHT + ("mostly_off",))),
    "lstm": (3, 3, 3, 3, (50, 50), LSTM3, COMBINED + ("minify_off_frame",), minimums(COMBINED + ("minify_off_frame",))),
})
# cases that additionally run through `slot_chain` and with the specialised instantiations on and off, bit for bit against the generic
# launches: every single edit (the measured ones too: bit identity does not depend on conditioning) and the combined ones.  All have the
# shipped shape, so by default they take the specialised kernels; the generic ones are reached through this leg.
EXECUTORS = SINGLE + ("combined", "combined_off_frame")

# name: (K, N, T, B, flags, options, wide library, edits, minimums); frame 50 x 50.  (Data seed 7: at seed 5 the fp32 oracle's own
# gradients under `saturated_presence` are 1.8e-4 from the fp64 ones, above a quarter of the 5e-4 bar; at 7 they are 6e-5.)
BWD_HW, BWD_SEED = (50, 50), 7
_OFF = COMBINED + ("minify_off_frame",)
BACKWARD = {e: (3, 3, 3, 3, {}, None, False, (e,), minimums((e,))) for e in SINGLE}
BACKWARD.update({
    "combined": (3, 3, 3, 3, {}, None, False, COMBINED, minimums(COMBINED)),
    "combined_off_frame": (3, 3, 3, 3, {}, None, False, _OFF, minimums(_OFF)),
})
# ... and every one of them again through the in-launch slot chain (sqair_chain.hip holds its own copy of the crop, the scale
# floors and the clamp); the oracle side is shared with the launches' case
BACKWARD.update({name + "_slot_chain": c[:5] + ({"slot_chain": 1},) + c[6:] for name, c in list(BACKWARD.items())})
BACKWARD["wide_n_what_64"] = (3, 3, 3, 3, dict(n_what=64), None, True, COMBINED + ("magnify_off_frame",),
                              minimums(COMBINED + ("magnify_off_frame",), NOT_BRIGHT + ("mostly_off",)))   # (the chain does not serve n_what > 50)
CLAMP_CASES = ("scale_clamp", "scale_clamp_slot_chain")
# first noise seed `stable_noise` tries, by the case's edits: 100 (the other suites') unless that draw is not kink-stable (below:
# `kink_recorder`; decided on the oracle alone by tests/test_latent_regimes.py)
BWD_NOISE_SEED0 = {("bright_decoder",): 106, ("floored_prior",): 106, ("scale_clamp",): 106, ("where_spread",): 106,
                   COMBINED + ("magnify_off_frame",): 103}


def bwd_noise_seed0(edits):
    return BWD_NOISE_SEED0.get(tuple(edits), 100)


GRAD_TIGHT, GRAD_LOOSE = 5e-4, 3e-3    # tests/pass_cases.py: TIGHT; LOOSE for the two `*.transform.scale_offset` scalars
GRAD_LOOSE_NAMES = ("disc.transform.scale_offset", "prop.transform.scale_offset")

# the stream, the carried training chunk, the particle filter and the forecast (sizes and seeds: the helpers of those suites)
STREAM = dict(K=2, N=3, T=12, B=3, hw=(50, 50), edits=COMBINED, chunks=([1] * 12, [4, 4, 4]), minimums=minimums(COMBINED))
STREAM_TRAIN = dict(flags=dict(k_particles=3, n_steps_per_image=2), edits=COMBINED,
                    minimums=dict(where_std_floor=4, what_std_small=2, saturated_logit=4))
SMC = dict(flags=dict(k_particles=4, n_steps_per_image=2), B=3, frames_per_step=1, frames=10, ess_frac=0.5,
           edits=("saturated_presence",), minimums=dict(saturated_logit=2))
FORECAST = dict(flags=dict(k_particles=3, n_steps_per_image=3), hw=(32, 40), B=3, S=4, Fn=6, edits=("floored_prior",),
                minimums=PRIOR_REACH)
GRAPH_FORWARD, GRAPH_TRAIN = "combined", "combined"


# ----------------------------------------------------------------------------- distances, in the suites' own scalings
SCALARS = ("elbo_vae", "elbo_iwae", "data_ll", "kl", "log_p_z", "log_q_z_given_x")
VECTORS = ("log_weights", "elbo_iwae_per_example")
OUTPUT_BAR, BOUND_BAR = 5e-4, 1e-4     # tests/pass_cases.check_against: every output scaled; the bounds relative


def output_distances(model, ref):
    """Per public output: max |model - ref| / max(|ref|, 1) (the scaling of `check_against`); model, ref: oracle models."""
    out = {}
    for k, v in ref.outputs.items():
        if not k.startswith("_"):
            want = _np(v)
            out[k] = float(np.abs(_np(model.outputs[k]) - want).max() / max(np.abs(want).max(), 1.0))
    return out


def bound_distances(model, ref):
    """The bounds in `check_against`'s scalings: the vectors as max |d| / max |ref|, the scalars as |d| / max(|ref|, 1)."""
    out = {}
    for k in VECTORS:
        want = _np(getattr(ref, k))
        out[k] = float(np.abs(_np(getattr(model, k)) - want).max() / max(np.abs(want).max(), 1e-30))
    for k in SCALARS:
        want = float(_np(getattr(ref, k)))
        out[k] = abs(float(_np(getattr(model, k))) - want) / max(abs(want), 1.0)
    return out


def same_decisions(model, ref):
    return all(np.array_equal(_np(getattr(model, k)), _np(getattr(ref, k))) for k in ("presence", "prop_pres", "disc_pres", "obj_id"))


def gradient_report(grads, ref_grads):
    """[(name, max |g - ref|, max |ref|)] over the reference's parameters: the `report` of tests/test_hip_backward.py."""
    rep = []
    for name, want in ref_grads.items():
        g = np.zeros_like(want) if grads.get(name) is None else np.asarray(grads[name], np.float64).reshape(want.shape)
        rep.append((name, float(np.abs(g - want).max()), float(np.abs(want).max())))
    return rep


def gradient_rel(report):
    """{name: error / max(|grad|max, 1e-4 of the pass's largest gradient)}: `check_report`'s `rel`."""
    gmax = max(s for _, _, s in report)
    return {n: e / max(s, 1e-4 * gmax) for n, e, s in report}


def oracle_grads(orc):
    return {k: (np.zeros(tuple(v.shape)) if v.grad is None else v.grad.detach().numpy().astype(np.float64)) for k, v in orc.P.items()}


def forecast_prior_counts(ref):
    """`prior_counts_of` on a rollout of tests/forecast_ref.py (its `_prior_*` extras: the prior every forecast frame samples from)."""
    n = ref["_prior_logit"].shape[0]
    return prior_counts_of([(ref["_prior_where_scale"][f], ref["_prior_what_scale"][f], ref["_prior_logit"][f],
                             ref["_prior_prev_presence"][f]) for f in range(n)])


# The clamp cases.  The reference clips the glimpse scale with `clip_preserve` (ops.py:33-42: forward max(s, 1e-4), gradient of the
# identity), and so do the kernels.  Below the clamp that path contributes sigmoid'(l) ~ 2e-5 times d target / d sc to the gradient
# of `disc.transform.l2.b[:2]`; a glimpse of scale 1e-4 samples one point of the frame, so d target / d sc is of order 1 to 10 and the
# clamp's contribution is ~1e-4 against gradients of ~30 that reach the two entries through the where log-probabilities and the
# recurrence: zero at the bar's resolution, whichever way the clip is differentiated (measured by tests/test_latent_regimes.py).  What
# the clamp cases pin on the device is that nothing BLOWS UP through 1 / sc = 1e4 (the insert's grid is (Xn - tx) / sx): the two
# entries must equal the oracle's within the parameter's bar.
CLAMP_CONTRIBUTION = 0.1    # of the bar: the most the clip's own path may contribute on the oracle


# ----------------------------------------------------------------------------- kinks of the bilinear samplers
# A bilinear sample is continuous in its coordinate but its DERIVATIVE jumps where the coordinate crosses an integer (another pair of
# taps).  A gradient case whose oracle has a sample coordinate closer to an integer than fp32 resolves is not a comparison of two
# computations of one gradient: the fp64 oracle differentiates on one side, an fp32 implementation may land on the other, and both
# are right.  At initialisation the jump is lost in the bar; where the learning signal is in the thousands (`bright_decoder`,
# `floored_prior`) it is not -- found with a crop row at 15 + 2.7e-7 pixels, which moved whole gradients by 1e-2 and is reproduced
# to three digits by nudging the ORACLE's coordinates by 2e-6.  So a gradient case also needs a kink-stable draw, decided on the
# oracle alone like the presence margin: every coordinate whose taps touch the source stays KINK_ULPS fp32 ulps (of the
# coordinate's own size) away from an integer.  Four ulps: the coordinate is the end of about four fp32 operations on the where
# logits (an activation, a product, a sum, a scaling), each good to half an ulp of a value no larger than the coordinate, doubled for
# the difference between an fp32 `where` and the oracle's.
# That count holds for the CROP grid 0.5 (L - 1) (sc g + tr + 1).  It does not hold for the INSERT grid 0.5 (G - 1) ((Xn - tx) / sx + 1)
# at small scales: one ulp of tx is amplified by 1 / sx, to about 1e-3 glimpse pixels at sx = 1e-4 ... 1e-3, far beyond any margin
# that a draw could meet.  In `scale_clamp` and `tiny_scale` the condition therefore UNDER-PROTECTS the insert coordinates: there fp32
# does not resolve on which side of a glimpse pixel a canvas pixel falls, the condition says nothing about it, and those cases stand
# on the measured agreement alone (a glimpse of that scale reaches at most a pixel or two of the canvas).
KINK_ULPS = 4.0


class kink_recorder(object):
    """Context manager: records, for every bilinear sample the oracle takes inside it (crops and inserts), the clearance of the
    closest coordinate to an integer in units of the margin (KINK_ULPS ulps of max(|x|, 1)); coordinates whose taps lie outside the
    source on both sides carry no weight and are left out.  `clearance` < 1: the draw is not kink-stable."""

    def __enter__(self):
        self.inner, self.worst = O.bilinear_gather, []

        def recorded(src, x, y):
            for v, L in ((x, src.shape[2]), (y, src.shape[1])):
                c = v.detach().double()
                inside = (c > -1.0) & (c < float(L))
                if bool(inside.any()):
                    margin = KINK_ULPS * 2.0 ** -23 * torch.clamp(c.abs(), min=1.0)
                    rel = torch.where(inside, (c - torch.round(c)).abs() / margin, torch.full_like(c, float("inf")))
                    i = int(rel.reshape(-1).argmin())
                    self.worst.append((float(rel.reshape(-1)[i]), float(c.reshape(-1)[i]), tuple(src.shape[1:])))
            return self.inner(src, x, y)
        O.bilinear_gather = recorded
        return self

    def __exit__(self, *exc):
        O.bilinear_gather = self.inner
        return False

    @property
    def clearance(self):
        return min(self.worst)[0] if self.worst else float("inf")

    def closest(self):
        w = min(self.worst)
        return "closest sample coordinate {!r} in a {} source: {:.2f} of the margin of {} fp32 ulps".format(w[1], w[2], w[0], KINK_ULPS)


def kink_clearance(P, cfg, obs, noise, nums=None):
    """One more fp64 pass of the oracle over the same inputs with its samplers recorded; returns the recorder."""
    orc = O.SqairOracle(P, cfg, torch.float64)
    with kink_recorder() as rec, torch.no_grad():
        orc.model(obs, noise, num=nums)
    return rec
