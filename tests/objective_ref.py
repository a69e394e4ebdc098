"""Reference for the objective and optimiser kernels (k_elbo, k_elbo_wide, k_elbo_bwd; k_rmsprop, k_add_l2), CPU only.

`reference` is the float64 statement, built on the oracle's functions (oracle/sqair_oracle.py: iwae, vimco_control_variate, vimco,
reinforce, ess) plus the importance-weighted mean of sqair/model.py:202-205 (mean over b of sum_k w_bk mean_t x_tbk); the gradients
of target / T with respect to log_w_t and disc_lp_t are autograd's.  `restate` writes the same formulas out once more with the
dtype as an argument: in float64 it must agree with `reference` (tests/test_objective_ref.py pins that), in float32 -- every
intermediate rounded, the frame sum in frame order -- its error against the reference is the yardstick the bars of
tests/test_objective_kernels.py come from (R.bar_from_fp32: 8 x the worst over a kernel's cases).  The restatement is never
compared with a kernel.  `mutate` names one deliberate mistake (MUTATIONS, OPT_MUTATIONS) made in the float32 restatement: the
power check demands that the GPU test's own cases and metric see each.

The metric, from the float64 reference alone (`scales`):
  log_weights[b, k]   / S_bk = sum_t |log_w_t[t, b, k]| + log K
  signal[b, k], elbo_per_ex[b]   / S_b = max_k S_bk (the control variate and the bound are reductions over the lane)
  elbo_vae, elbo_iwae   / max_b S_b;  target   / max_b S_b (1 + max_bk sum_t |disc_lp_t|) / T  (d(sig dl) = dsig |dl| + |sig| ddl)
  iw[b, k]   / W_b = max(1, max_k |LW_bk|): dw_k = w_k (dLW_k - sum_j w_j dLW_j), so |dw| <= max |dLW| / 2 -- the weights inherit
      the ABSOLUTE error of the summed log-weights, eps |LW|; an unscaled bar would be set by the one case with the largest |LW|
  ess   / mean_b W_b ess_b  (d ess_b <= 4 max|dLW| ess_b);  mean q   / mean_b W_b sum_k w_bk mean_t |x_tbk|
  g_log_w_t[t, b, k]   / W_b / (B T);  g_disc_lp_t[t, b, k]   / S_b / (B K T)
Under VIMCO with K = 1 the reference's signal and target are NaN (0 / 0 in the leave-one-out mean); they are compared as "both NaN".

CASES / build_case (the covering list of the GPU test) need no GPU; nor do the optimiser's cases (rms_cases, RMS_*, L2_*)."""
import math

import numpy as np
import torch

from oracle import sqair_oracle as O
from sqair_amd.train import rmsprop_reference
from tests import slot_adjoint_ref as R

F32, F64 = np.float32, np.float64
MUTATIONS = ("loo_divided_by_K", "own_weight_in_loo_sum", "last_particle_dropped", "frames_after_first_chunk_dropped",
             "last_partial_chunk_twice", "lane_b16_gets_lane_b", "means_not_divided_by_T", "mean_q_reads_q_minus_1", "ess_over_BK",
             "target_not_divided_by_T", "signal_sign_flipped", "disc_lp_counted_although_null")
OPT_MUTATIONS = ("eps_outside_sqrt", "ms_after_momentum", "grad_scale_once", "tail_skipped", "l2_on_grad")
REGIMES = ("dominated", "near_equal", "moderate", "small", "two_leaders", "bit_equal", "one_far_below")
OUTPUTS = ("log_weights", "elbo_per_ex", "iw", "signal", "scalars")          # the nullable outputs, in argument order
SCALARS = ("elbo_vae", "elbo_iwae", "target", "ess")
PARITY_FILE = "objective_parity.json"
PARITY_NOTE = ("per kernel, case and output of tests/test_objective_kernels.py and tests/test_optimiser_kernels.py: the kernel's largest "
               "scaled error against the float64 reference, the bar (8 x the worst error of the same formulas in float32 over the "
               "kernel's cases), the float32 restatement's own error in this case; `bars`: per kernel and output the float32 figure "
               "the bar comes from; `worst_ratio`: per kernel the largest err / bar")


def fpi_of(K):
    """Frames per load instruction of k_elbo (1 in k_elbo_wide)."""
    return max(1, 64 // K)


# ------------------------------------------------------------------------------------------------ the float64 reference
def reference(lw_t, dl_t, xs, reinforce):
    """lw_t [T, B, K] float32 (dl_t the same or None, xs a list of such).  Everything float64 numpy."""
    T = lw_t.shape[0]
    a = torch.tensor(lw_t, dtype=torch.float64, requires_grad=True)
    d = torch.tensor(np.zeros_like(lw_t) if dl_t is None else dl_t, dtype=torch.float64, requires_grad=True)
    LW, DL = a.sum(0), d.sum(0)
    elbo = O.iwae(LW)
    iw = torch.softmax(LW, -1)
    signal = LW if reinforce else LW - O.vimco_control_variate(LW)
    target = (O.reinforce if reinforce else O.vimco)(LW, DL, elbo) / T
    out = dict(log_weights=LW, elbo_per_ex=elbo, iw=iw, signal=signal,
               scalars=torch.stack([LW.mean(), elbo.mean(), target, O.ess(iw)]),
               means=torch.stack([(iw * torch.tensor(x, dtype=torch.float64).mean(0)).sum(-1).mean() for x in xs]) if xs else torch.zeros(0))
    if bool(torch.isfinite(target)):
        g = torch.autograd.grad(target, [a, d], allow_unused=True)
        out["g_log_w_t"] = g[0]
        out["g_disc_lp_t"] = torch.zeros_like(d) if g[1] is None else g[1]
    return {k: v.detach().numpy().astype(F64) for k, v in out.items()}


def scales(lw_t, dl_t, xs, ref):
    T, B, K = lw_t.shape
    S = np.abs(lw_t.astype(F64)).sum(0) + math.log(K)                            # [B, K]
    S_b = S.max(-1)
    W_b = np.maximum(1.0, np.abs(ref["log_weights"]).max(-1))
    dl_abs = 0.0 if dl_t is None else float(np.abs(dl_t.astype(F64)).sum(0).max())
    iw = ref["iw"]
    ess_b = iw.sum(-1) ** 2 / (iw ** 2).sum(-1)
    return dict(log_weights=S, signal=S_b[:, None] + 0 * S, elbo_per_ex=S_b, iw=W_b[:, None] + 0 * S,
                scalars=np.array([S_b.max(), S_b.max(), S_b.max() * (1.0 + dl_abs) / T, float((W_b * ess_b).mean())]),
                means=np.array([float((W_b * (iw * np.abs(x.astype(F64)).mean(0)).sum(-1)).mean()) for x in xs]),
                g_log_w_t=np.broadcast_to(W_b[None, :, None] / (B * T), lw_t.shape),
                g_disc_lp_t=np.broadcast_to(S_b[None, :, None] / (B * K * T), lw_t.shape))


# ------------------------------------------------------------------------------------------------ the restatement
def _frame_sum(x_t, dt, K, mutate):
    """Sum over frames in frame order, every partial sum in dt."""
    T = x_t.shape[0]
    fpi = fpi_of(K)
    frames = list(range(T))
    if mutate == "frames_after_first_chunk_dropped":
        frames = frames[:fpi]
    if mutate == "last_partial_chunk_twice" and T % fpi:
        frames = frames + frames[T - T % fpi:]
    acc = torch.zeros(x_t.shape[1:], dtype=dt)
    for t in frames:
        acc = acc + x_t[t]
    if mutate == "lane_b16_gets_lane_b":
        src = [b - 16 if b % 32 >= 16 else b for b in range(acc.shape[0])]
        acc = acc[src]
    return acc


def restate(lw_t, dl_t, xs, reinforce, dt=torch.float32, mutate=None):
    """The formulas of `reference` written out in dtype dt (targets.py:38-75, model.py:150-158, :202-205, ops.py:52-59), the
    gradients as the closed forms -iw / (B T) and -signal / (B K T).  Returns float64 numpy arrays of dt's values."""
    T, B, K = lw_t.shape
    c = lambda v: torch.tensor(float(v), dtype=dt)
    LW = _frame_sum(torch.tensor(lw_t, dtype=dt), dt, K, mutate)
    counted = dl_t if (dl_t is not None or mutate != "disc_lp_counted_although_null") else lw_t
    DL = torch.zeros_like(LW) if counted is None else _frame_sum(torch.tensor(counted, dtype=dt), dt, K, mutate)
    live = LW[:, :K - 1] if (mutate == "last_particle_dropped" and K > 1) else LW
    mx = live.max(-1, keepdim=True).values
    ex = torch.exp(live - mx)
    se = ex.sum(-1, keepdim=True)
    elbo = (mx + torch.log(se))[:, 0] - torch.log(c(K))
    iw = ex / se
    if live.shape != LW.shape:
        iw = torch.cat([iw, torch.zeros(B, 1, dtype=dt)], -1)
    # the control variate: entry k replaced by the mean of the others, log-mean-exp over the K entries
    s = LW.sum(-1, keepdim=True)
    abo = (s if mutate == "own_weight_in_loo_sum" else s - LW) / (c(K) if mutate == "loo_divided_by_K" else c(K) - c(1))
    base = LW[:, :, None] + torch.diag_embed(abo - LW)
    m2 = base.max(-2, keepdim=True).values
    cv = (m2 + torch.log(torch.exp(base - m2).sum(-2, keepdim=True)))[:, 0, :] - torch.log(c(K))
    signal = LW if reinforce else LW - cv
    if mutate == "signal_sign_flipped":
        signal = -signal
    target = (-elbo[:, None] - signal * DL).sum() / c(B * K)
    if mutate != "target_not_divided_by_T":
        target = target / c(T)
    ess = (iw.sum(-1) ** 2 / (iw ** 2).sum(-1)).sum() / c(B * K if mutate == "ess_over_BK" else B)
    means = []
    for q in range(len(xs)):
        x = xs[(q - 1) % len(xs)] if mutate == "mean_q_reads_q_minus_1" else xs[q]
        xm = _frame_sum(torch.tensor(x, dtype=dt), dt, K, mutate)
        if mutate != "means_not_divided_by_T":
            xm = xm / c(T)
        means.append((iw * xm).sum(-1).sum() / c(B))
    out = dict(log_weights=LW, elbo_per_ex=elbo, iw=iw, signal=signal,
               scalars=torch.stack([LW.sum() / c(B * K), elbo.sum() / c(B), target, ess]),
               means=torch.stack(means) if means else torch.zeros(0, dtype=dt),
               g_log_w_t=(-iw / (c(B) * c(T)))[None].expand(T, B, K),
               g_disc_lp_t=(-signal / (c(B) * c(K) * c(T)))[None].expand(T, B, K))
    return {k: v.double().numpy() for k, v in out.items()}


def elbo_bwd_restate(iw, sig, T, B, K, dt):
    """k_elbo_bwd's two outputs from given float32 iw / signal [B, K], evaluated in numpy dtype dt: [T, B, K] each, as float64."""
    g_lw = -iw.astype(dt) / (dt(B) * dt(T))
    g_dl = -sig.astype(dt) / (dt(B) * dt(K) * dt(T))
    return {k: np.broadcast_to(v.astype(F64)[None], (T, B, K)) for k, v in (("g_log_w_t", g_lw), ("g_disc_lp_t", g_dl))}


def nan_pattern_ok(got, ref):
    """Where the reference is NaN the other must be NaN, and nowhere else."""
    return bool(np.array_equal(np.isnan(got), np.isnan(ref)))


def errors(got, ref, sc, names=None):
    """{output: worst scaled error}; the scalars and the means per entry ('scalars.ess', 'means').  Entries NaN in the reference
    (K = 1 under VIMCO) must be NaN and are not measured; anything else non-finite is an infinite error."""
    e = {}
    for k in (ref if names is None else names):
        g, r, s = np.asarray(got[k], F64), np.asarray(ref[k], F64), np.asarray(sc[k], F64)
        if k == "scalars":
            for i, n in enumerate(SCALARS):
                e["scalars." + n] = _err(g[i:i + 1], r[i:i + 1], s[i:i + 1])
        elif k != "means" or r.size:
            e[k] = _err(g, r, s)
    return e


def _err(g, r, s):
    if not nan_pattern_ok(g, r):
        return float("inf")
    ok = ~np.isnan(r)
    return R.row_scaled_error(g[ok], r[ok], s[ok]) if ok.any() else 0.0


# ------------------------------------------------------------------------------------------------ the cases
def _covering_cases():
    cases = {}
    # disc_lp_t, vi_target and the NULL output are dealt with the co-prime periods 3, 4 and 7, so their combinations spread
    Bs, NMs, NULLS = (1, 16, 17, 33, 50), (0, 1, 3, 7, 8), (None,) + OUTPUTS + (None,)
    i = 0
    for K in (1, 2, 5, 13, 32, 33, 64, 65, 100, 256):
        fpi = fpi_of(K)
        for tk, T in (("1", 1), ("fpi", fpi), ("fpi+1", fpi + 1), ("2fpi+3", 2 * fpi + 3)):
            B, nm = Bs[(i + i // 5) % 5], NMs[(2 * i + i // 5) % 5]
            while T * B * K * (2 + nm) > 100000 and B > 1:              # the largest case stays at a few hundred KB
                B = Bs[Bs.index(B) - 1]
            cases["K%d T%d(%s) B%d m%d %s %s -%s" % (K, T, tk, B, nm, "dl" if i % 3 else "nodl", "reinforce" if i % 4 == 1 else "vimco",
                                                   NULLS[i % 7] or "none")] = dict(
                K=K, T=T, B=B, n_means=nm, disc=bool(i % 3), reinforce=int(i % 4 == 1), null=NULLS[i % 7], wide=False, seed=i,
                null_means=nm == 0 and i % 2 == 0)       # n_means = 0: iw_means_in and iw_means_out may both be NULL
            i += 1
    # the wide build compiles the same source
    cases["wide K5 T13(fpi+1) B33 m7 dl vimco -none"] = dict(K=5, T=13, B=33, n_means=7, disc=True, reinforce=0, null=None, wide=True, seed=90,
                                                             null_means=False)
    cases["wide K100 T2(fpi+1) B17 m3 dl vimco -none"] = dict(K=100, T=2, B=17, n_means=3, disc=True, reinforce=0, null=None, wide=True, seed=91,
                                                              null_means=False)
    return cases


CASES = _covering_cases()
# sqair_elbo -> sqair_elbo_bwd: every K 5, 33, 64, 100 case of the list that passes iw and signal
CHAINED = sorted(n for n, c in CASES.items() if c["K"] in (5, 33, 64, 100) and c["null"] not in ("iw", "signal"))
BWD_SHAPES = ((1, 1, 1), (3, 17, 5), (1, 4, 64), (257, 1, 1), (3, 70, 33))      # (T, B, K): T B K = 1, 255, 256, 257, 3 * 33 * 70


def draw_lane(rng, regime, T, K):
    """Per-frame log-weights [T, K] of one lane, float64."""
    if regime == "dominated":
        return rng.normal(500.0, 30.0, (T, K))
    if regime == "near_equal":
        return rng.normal(-700.0, 0.01, (T, K))
    if regime == "moderate":
        return rng.normal(-80.0, 1.0, (T, K))
    if regime == "small":
        return rng.normal(0.0, 0.5, (T, K))
    if regime == "two_leaders":          # the same frames for every particle; frame 0 carries the gaps
        x = np.repeat(rng.normal(-40.0, 1.0, (T, 1)), K, 1)
        gap = -50.0 - rng.uniform(0.0, 5.0, K)
        lead = rng.permutation(K)[:2]
        gap[lead[0]] = 0.0
        if K > 1:
            gap[lead[1]] = -rng.uniform(0.0, 0.1)
        x[0] += gap
        return x
    if regime == "bit_equal":
        return np.repeat(rng.normal(-80.0, 1.0, (T, 1)), K, 1)
    assert regime == "one_far_below"
    x = rng.normal(-80.0, 1.0, (T, K))
    if K > 1:
        x[0, rng.integers(K)] -= 200.0
    return x


def lane_regimes(B, seed):
    return [REGIMES[(b + seed) % len(REGIMES)] for b in range(B)]


def draw_inputs(rng, T, B, K, n_means, disc, seed):
    regimes = lane_regimes(B, seed)
    lw_t = np.stack([draw_lane(rng, rg, T, K) for rg in regimes], 1).astype(F32)
    dl_t = None
    if disc:
        dl = rng.normal(-3.0, 2.0, (T, B, K))
        dl[rng.uniform(size=dl.shape) < 0.1] = 0.0
        dl_t = dl.astype(F32)
    xs = [(rng.standard_normal((T, B, K)) * 10.0 ** rng.uniform(-2, 1, (T, B, K))).astype(F32) for _ in range(8)]   # eight distinct arrays
    return lw_t, dl_t, xs, regimes


def build_case(name):
    c = CASES[name]
    T, B, K, nm = c["T"], c["B"], c["K"], c["n_means"]
    rng = np.random.default_rng(7000 + c["seed"])
    lw_t, dl_t, xs, regimes = draw_inputs(rng, T, B, K, nm, c["disc"], c["seed"])
    ref = reference(lw_t, dl_t, xs[:nm], c["reinforce"])
    nan_ok = K == 1 and not c["reinforce"]
    for k, v in ref.items():                 # the reference is finite for every lane drawn; K = 1 under VIMCO is the one exception
        bad = ~np.isfinite(v)
        if nan_ok and k == "signal":
            assert np.isnan(v).all()
        elif nan_ok and k == "scalars":
            assert np.isnan(v[2]) and np.isfinite(np.delete(v, 2)).all()
        else:
            assert not bad.any(), (name, k, [regimes[b] for b in np.argwhere(bad)[:, 0 if v.ndim < 3 else 1][:3]] if v.ndim else None)
    sc = scales(lw_t, dl_t, xs[:nm], ref)
    r32 = restate(lw_t, dl_t, xs[:nm], c["reinforce"])
    names = [k for k in ("log_weights", "elbo_per_ex", "iw", "signal", "scalars", "means") if k != c["null"]]
    chained = name in CHAINED
    return dict(c, lw_t=lw_t, dl_t=dl_t, xs=xs, regimes=regimes, ref=ref, scales=sc, names=names, chained=chained,
                err32=errors(r32, ref, sc, names),
                bwd_err32=errors(r32, ref, sc, ["g_log_w_t", "g_disc_lp_t"]) if chained else {})


def kernel_of(case):
    return "k_elbo_wide" if CASES[case]["K"] > 64 else "k_elbo"


def worst32(built, kernel):
    """Per output of `kernel` ('k_elbo' | 'k_elbo_wide'; the chained gradients with it): the worst error of the float32 restatement
    over the kernel's cases -- what its bars are 8 x of."""
    worst = {}
    for name, c in built.items():
        if kernel_of(name) == kernel:
            for k, e in list(c["err32"].items()) + list(c["bwd_err32"].items()):
                worst[k] = max(worst.get(k, 0.0), e)
    return worst


def mutated_errors(case, built, mutate):
    c = built
    r = restate(c["lw_t"], c["dl_t"], c["xs"][:c["n_means"]], c["reinforce"], mutate=mutate)
    return errors(r, c["ref"], c["scales"], c["names"] + (["g_log_w_t", "g_disc_lp_t"] if c["chained"] else []))


def build_bwd_case(shape):
    """k_elbo_bwd on its own: iw / signal are float32 roundings of the reference's for mixed lanes; the kernel's chain is not
    involved.  An element's error is divided by the largest reference magnitude of its (frame, lane): iw reaches into the float32
    denormals, where a relative error per element would measure the number format."""
    T, B, K = shape
    rng = np.random.default_rng(8000 + T * B * K)
    lw_t, _, _, _ = draw_inputs(rng, 1, B, K, 0, False, T)
    ref = reference(lw_t, None, [], 1 if K == 1 else 0)
    iw, sig = ref["iw"].astype(F32), ref["signal"].astype(F32)
    want = elbo_bwd_restate(iw, sig, T, B, K, F64)
    got32 = elbo_bwd_restate(iw, sig, T, B, K, F32)
    return dict(T=T, B=B, K=K, iw=iw, sig=sig, ref=want, err32={k: R.row_scaled_error(got32[k], want[k]) for k in want})


# ------------------------------------------------------------------------------------------------ the optimiser
RMS_N = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 3 * 1024 + 1)
RMS_ALIGN = ("aligned", "theta", "grad", "ms", "mom")                 # which buffer starts one word off a 16-byte boundary
RMS_HYPER = (dict(lr=1e-3, decay=0.9, momentum=0.9, eps=1e-10), dict(lr=3e-2, decay=0.95, momentum=0.0, eps=1e-6))
RMS_SCALES = (1.0, 0.5, 0.125)
L2_N = (1, 255, 256, 257, 70001)
L2_WEIGHTS = (1e-4, 0.5)


def rms_cases():
    """{name: (n, which buffer is off by one word, hyper-parameters, grad_scale)}: every n on the float4 path and on the scalar
    path (any one buffer off takes the whole launch there), n = 3 and n = 1025 with each of the four buffers off in turn, the
    others with one, dealt round like the hyper-parameter sets and grad scales."""
    cases = {}
    for i, n in enumerate(RMS_N):
        for j, al in enumerate(RMS_ALIGN if n in (3, 1025) else ("aligned", RMS_ALIGN[1 + i % 4])):
            h = (i + j) % 2
            cases["n%d %s h%d gs%g" % (n, al, h, RMS_SCALES[(i + j) % 3])] = (n, al, RMS_HYPER[h], RMS_SCALES[(i + j) % 3])
    return cases


def rms_state(n, seed):
    """theta, grad, ms, mom (float32): ms from {0, 1e-12, 1, 1e6} per element, g = N(0, 1) x 10^U(-4, 2) with exact zeros (elements
    with ms = 0 and g = 0 among them: 0 / sqrt(eps) = 0), mom mixed."""
    rng = np.random.default_rng(9000 + seed)
    theta = rng.standard_normal(n).astype(F32)
    g = rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 2, n)
    g[rng.uniform(size=n) < 0.2] = 0.0
    ms = rng.choice(np.array([0.0, 1e-12, 1.0, 1e6]), n)
    if n >= 4:
        g[1], ms[1] = 0.0, 0.0
    mom = rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 0, n)
    mom[rng.uniform(size=n) < 0.2] = 0.0
    return theta, g.astype(F32), ms.astype(F32), mom.astype(F32)


def rms_step(theta, g, ms, mom, hyper, grad_scale, dt=F64, mutate=None):
    """One step in numpy dtype dt: (theta, ms, mom).  float64 without a mutation is sqair_amd.train.rmsprop_reference."""
    lr, rho, mu, eps, gs = [dt(hyper[k]) for k in ("lr", "decay", "momentum", "eps")] + [dt(grad_scale)]
    theta, g, ms, mom = (np.asarray(v).astype(dt) for v in (theta, g, ms, mom))
    if dt is F64 and mutate is None:
        return rmsprop_reference(theta, g * gs, ms, mom, lr, rho, mu, eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        gg = g * gs
        g2 = g * g * gs if mutate == "grad_scale_once" else gg * gg
        new_ms = rho * ms + (dt(1) - rho) * g2
        den_ms = ms if mutate == "ms_after_momentum" else new_ms
        den = np.sqrt(den_ms) + eps if mutate == "eps_outside_sqrt" else np.sqrt(den_ms + eps)
        new_mom = mu * mom + lr * gg / den
        new_theta = theta - new_mom
    if mutate == "tail_skipped" and len(theta) % 4:
        keep = len(theta) - len(theta) % 4
        new_theta[keep:], new_ms[keep:], new_mom[keep:] = theta[keep:], ms[keep:], mom[keep:]
    return new_theta, new_ms, new_mom


def rms_errors(got, ref, state, hyper):
    """theta's error is divided by max(|theta|, |mom|, lr) of the element; ms and mom are relative, element by element."""
    theta, _, _, mom = (np.asarray(v, F64) for v in state)
    t_scale = np.maximum(np.maximum(np.abs(theta), np.abs(mom)), hyper["lr"])
    return dict(theta=R.row_scaled_error(got[0], ref[0], t_scale), ms=R.row_scaled_error(got[1], ref[1], np.abs(ref[1])),
                mom=R.row_scaled_error(got[2], ref[2], np.abs(ref[2])))


def l2_state(n, seed):
    rng = np.random.default_rng(9500 + seed)
    theta = (rng.standard_normal(n) * 10.0 ** rng.uniform(-2, 1, n)).astype(F32)
    grad = (rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 2, n)).astype(F32)
    grad[rng.uniform(size=n) < 0.1] = 0.0
    return theta, grad


def l2_step(theta, grad, l2, dt=F64, mutate=None):
    theta, grad = np.asarray(theta).astype(dt), np.asarray(grad).astype(dt)
    return grad + dt(l2) * (grad if mutate == "l2_on_grad" else theta)


def l2_error(got, theta, grad, l2):
    """Relative to the float64 sum of the absolute terms |grad| + l2 |theta|."""
    ref = l2_step(theta, grad, l2)
    return R.row_scaled_error(got, ref, np.abs(np.asarray(grad, F64)) + l2 * np.abs(np.asarray(theta, F64)))


def rms_worst32():
    """Per output of k_rmsprop: the worst error of the float32 restatement of one step over rms_cases()."""
    worst = {}
    for i, (n, _, hyper, gs) in enumerate(rms_cases().values()):
        st = rms_state(n, i)
        for k, v in rms_errors(rms_step(*st, hyper, gs, dt=F32), rms_step(*st, hyper, gs), st, hyper).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


def rms_three_steps(n, seed, hyper, gs, dt):
    """Three steps carrying the state in dt (fresh gradients each step, float32 values): (theta, ms, mom) and the gradients used."""
    theta, g, ms, mom = rms_state(n, seed)
    grads = [g] + [rms_state(n, seed + 100 * (1 + i))[1] for i in range(2)]
    st = (theta.astype(dt), ms.astype(dt), mom.astype(dt))
    for g in grads:
        st = rms_step(st[0], g, st[1], st[2], hyper, gs, dt=dt)
    return st, grads


def l2_worst32():
    return max(l2_error(l2_step(*l2_state(n, i), l2, dt=F32), *l2_state(n, i), l2) for i, n in enumerate(L2_N) for l2 in L2_WEIGHTS)
