"""Reference for the log-probability kernels (k_logprob, k_logprob_bwd).

`forward` restates k_logprob on the oracle's own functions (oracle/sqair_oracle.py: normal_log_prob, bernoulli_log_prob, softplus,
elu, fill_triangular, bernoulli_to_modified_geometric, num_steps_log_prob, vanilla_rnn, linear, mlp_1hidden_out,
SqairOracle.mvn_tril_log_prob, the prior-type rules of propagate_prior, the loop of recurrent_normal_log_prob) from a tape in the
kernel's record layout; the adjoint is autograd of sum over (frame, row) of g_lw (pz - qz) + g_dl disc_lp.  No derivative is
written down.  The same functions run in float64 (the reference) and in float32 (the yardstick the bars of
tests/test_logprob_kernels.py come from).  tests/test_logprob_ref.py pins all of it on the CPU against SqairOracle.timestep and
central differences.

Saved activations are inverted to obtain their leaves, as in tests/slot_adjoint_ref.py: the kernels read discovery's PROB and
report the gradient in LOGIT, so that leaf is logit(PROB_fp32) evaluated in the piece's dtype.

A tape (numpy, float32 values): rec_p, rec_d [T, R, N, W]; rec_m [T + 1, R, N, W] (frame f reads rec_m[f], the merged records of
f - 1); pstats [T, R, N, 9 + 2 n_what] = [logit | where_loc 4 | what_loc | where_scale 4 | what_scale], raw; spre [T, R, 128];
t [T, R] the time of every (frame, row); params {oracle name: array} with 'disc.rn.cond.w:e' = row 4 + n_hidden of disc.rn.cond.w.

`mutate` names one deliberate mistake (MUTATIONS): the power check of tests/test_logprob_ref.py applies each to the float32
evaluation and demands that the GPU test's own cases see it."""
import numpy as np
import torch

from oracle import sqair_oracle as O
from tests.slot_adjoint_ref import MIN_STD, T as _T, adjoints, leaf, logit, where_tril

REC_FIELDS = ("where", "what", "logit", "where_loc", "where_scale", "what_loc", "what_scale")   # the differentiable record fields
Z_FIELDS = ("where", "what", "logit")
COLS = dict(where="WHERE", what="WHAT", logit="LOGIT", where_loc="WHERE_LOC", where_scale="WHERE_SCALE", what_loc="WHAT_LOC",
            what_scale="WHAT_SCALE")
# the fifteen segments k_logprob_bwd stages (SmallParamTab), by oracle name
SMALL_PARAMS = ("disc.rn.readout.w", "disc.rn.readout.b", "disc.rn.i2h.w", "disc.rn.i2h.b", "disc.rn.h2h.w", "disc.rn.h2h.b",
                "disc.rn.cond.w:e", "disc.rn.init_sample", "disc.steps_prior.l0.w", "disc.steps_prior.l0.b", "disc.steps_prior.l1.w",
                "disc.steps_prior.l1.b", "disc.step_prior_bias", "disc.step_prior_timestep_bias", "prop.cholesky_scale")
RN_PARAMS, CAT_PARAMS = SMALL_PARAMS[:8], SMALL_PARAMS[8:14]
MUTATIONS = ("cholesky_swapped", "t_row_ignored", "rec_m_late", "guided_as_rnn", "stop_term_dropped", "absent_e_path_dropped",
             "where_prior_reads_own_sample", "what_column_64_dropped")
PER_SLOT = ("prop_what_log_prob", "prop_where_log_prob", "prop_what_prior_log_prob", "prop_where_prior_log_prob", "prop_prob",
            "disc_what_log_prob", "disc_where_log_prob", "disc_what_prior_log_prob", "disc_where_prior_log_prob")
PER_ROW = ("prop_log_prob", "prop_prior_log_prob", "disc_log_prob", "disc_prior_log_prob", "step_log_prob", "discrete_log_prob")
REDUCED = ("qz", "pz", "disc_lp")
EXACT = ("prop_pres", "disc_pres", "num_prop_steps_per_sample", "num_disc_steps_per_sample")


def width(L, name, nw):
    return nw if name.startswith("what") else (4 if name.startswith("where") else 1)


def field(rec, L, name, nw):
    """Column block `name` of records [..., W]; one-column fields lose the axis."""
    c = L[COLS.get(name, name)]
    w = width(L, name, nw)
    return rec[..., c:c + w] if name.startswith(("what", "where")) else rec[..., c]


def used_params(cfg):
    """The small parameters the configuration's log-probabilities depend on."""
    return (RN_PARAMS if cfg.rec_where_prior else ()) + (CAT_PARAMS if cfg.disc_prior_type == "cat" else ()) + ("prop.cholesky_scale",)


def make_leaves(tape, L, cfg, dtype, mutate=None):
    """(leaves, constants) of a tape.  Leaves: 'p.<field>', 'd.<field>' (d.logit = logit(PROB)), 'm.where / what / logit' where the
    prior type reads them, 'ps', 'spre' (recurrent where prior), 'P:<name>' the small parameters in use."""
    N, nw = tape["rec_p"].shape[2], (tape["pstats"].shape[-1] - 9) // 2
    Tn = tape["rec_p"].shape[0]
    lv = {}
    for f in REC_FIELDS:
        lv["p." + f] = leaf(field(tape["rec_p"], L, f, nw), dtype)
        if f != "logit":
            lv["d." + f] = leaf(field(tape["rec_d"], L, f, nw), dtype)
    lv["d.logit"] = logit(_T(field(tape["rec_d"], L, "PROB", nw), dtype)).requires_grad_(True)
    rec_m = tape["rec_m"][1:Tn + 1] if mutate == "rec_m_late" else tape["rec_m"][:Tn]
    ptype = "rnn" if (mutate == "guided_as_rnn" and cfg.prop_prior_type == "guided") else cfg.prop_prior_type
    if ptype != "rnn":
        for f in Z_FIELDS:
            lv["m." + f] = leaf(field(rec_m, L, f, nw), dtype)
    lv["ps"] = leaf(tape["pstats"], dtype)
    if cfg.rec_where_prior:
        lv["spre"] = leaf(tape["spre"], dtype)
    for name in used_params(cfg):
        lv["P:" + name] = leaf(tape["params"][name], dtype)
    times = np.asarray(tape["t_ignored"] if mutate == "t_row_ignored" else tape["t"])
    c = dict(cfg=cfg, N=N, nw=nw, ptype=ptype, p_pres=_T(field(tape["rec_p"], L, "PRES", nw), dtype),
             d_pres=_T(field(tape["rec_d"], L, "PRES", nw), dtype), m_pres=_T(field(rec_m, L, "PRES", nw), dtype),
             later=torch.as_tensor(times > 0))
    return lv, c


def where_prior_log_prob(P, samples, spre, e, cond_e, own_sample=False):
    """SqairOracle.recurrent_normal_log_prob with the conditioning's pre-activation given: state = elu(spre + e cond_w[e row]),
    never advanced; step k reads the sample of step k - 1 (the trainable init_sample at k = 0)."""
    state = O.elu(spre + e * cond_e)
    sample = P["disc.rn.init_sample"].reshape(-1).expand(samples.shape[:-2] + (4,))
    lps = []
    for k in range(samples.shape[-2]):
        if own_sample:
            sample = samples[..., k, :]
        o = O.vanilla_rnn(P, "disc.rn", sample, state)
        st = O.linear(P, "disc.rn.readout", o)
        loc, scale = st[..., :4], O.softplus(st[..., 4:]) + MIN_STD
        sample = samples[..., k, :]
        lps.append(O.normal_log_prob(sample, loc, scale))
    return torch.stack(lps, -2)


def forward(lv, c, mutate=None):
    """Everything k_logprob emits, [T, R, ...] each, plus 'abs:<name>' for the reduced scalars (REDUCED, PER_ROW): the sums of the
    absolute values of the terms they are sums of."""
    cfg, N, nw, ptype = c["cfg"], c["N"], c["nw"], c["ptype"]
    P = {k[2:]: v for k, v in lv.items() if k.startswith("P:")}
    dt = lv["ps"].dtype
    pres, pres_tm1, dpres = c["p_pres"], c["m_pres"], c["d_pres"]
    col = torch.ones(nw, dtype=dt)
    if mutate == "what_column_64_dropped" and nw >= 64:
        col[63] = 0.0
    # ---- propagation: PropagatePrior after its Linear (oracle.propagate_prior), then Propagate._compute_log_probs (oracle.propagate)
    ps = lv["ps"]
    p_logit = ps[..., 0] + cfg.prop_prior_step_bias
    p_logit = pres_tm1 * p_logit + (pres_tm1 - 1.0) * 88.0
    pw_loc, pa_loc = ps[..., 1:5], ps[..., 5:5 + nw]
    pw_scale = O.softplus(ps[..., 5 + nw:9 + nw]) + MIN_STD
    pa_scale = O.softplus(ps[..., 9 + nw:9 + 2 * nw]) + MIN_STD
    if ptype == "rw":
        pw_loc, pa_loc, p_logit = lv["m.where"], lv["m.what"], lv["m.logit"] + 0.1 * p_logit
    elif ptype == "guided":
        pw_loc = lv["m.where"] + 0.1 * pw_loc
        pa_loc = lv["m.what"] + 0.1 * pa_loc
        p_logit = lv["m.logit"] + 0.1 * p_logit
    q_what = (O.normal_log_prob(lv["p.what"], lv["p.what_loc"], lv["p.what_scale"]) * col).sum(-1)
    q_where = O.SqairOracle.mvn_tril_log_prob(lv["p.where"], lv["p.where_loc"], where_tril(P["prop.cholesky_scale"], lv["p.where_scale"]))
    q_pres = O.bernoulli_log_prob(pres, lv["p.logit"])
    p_what = (O.normal_log_prob(lv["p.what"], pa_loc, pa_scale) * col).sum(-1)
    p_where = O.normal_log_prob(lv["p.where"], pw_loc, pw_scale).sum(-1)
    p_pres = O.bernoulli_log_prob(pres, p_logit)
    m = pres_tm1 * pres
    out = dict(prop_what_log_prob=q_what * m, prop_where_log_prob=q_where * m, prop_what_prior_log_prob=p_what * m,
               prop_where_prior_log_prob=p_where * m, prop_prob=torch.exp(q_pres) * pres_tm1, prop_pres=pres,
               prop_log_prob=(q_pres * pres_tm1).sum(-1), prop_prior_log_prob=(p_pres * pres_tm1).sum(-1),
               num_prop_steps_per_sample=pres.sum(-1))
    e = ((torch.sigmoid(p_logit) - 0.5) / N).sum(-1, keepdim=True)                        # SqairOracle.timestep: exp_steps
    # ---- discovery: Discover._compute_log_probs / _make_priors (oracle.discover)
    joint = O.bernoulli_to_modified_geometric(torch.sigmoid(lv["d.logit"]))
    n = dpres.sum(-1)
    q_num = O.num_steps_log_prob(joint, n)
    if mutate == "stop_term_dropped":
        idx = n.long().clamp(max=N - 1).unsqueeze(-1)
        stop = torch.where(n < N, torch.log1p(-torch.sigmoid(lv["d.logit"]).gather(-1, idx).squeeze(-1)), torch.zeros_like(n))
        q_num = q_num - stop + stop.detach()
    dq_what = (O.normal_log_prob(lv["d.what"], lv["d.what_loc"], lv["d.what_scale"]) * col).sum(-1) * dpres
    dq_where = O.normal_log_prob(lv["d.where"], lv["d.where_loc"], lv["d.where_scale"]).sum(-1) * dpres
    dp_what = (O.normal_log_prob(lv["d.what"], torch.zeros((), dtype=dt), torch.ones((), dtype=dt)) * col).sum(-1) * dpres
    if cfg.rec_where_prior:
        dp_where = where_prior_log_prob(P, lv["d.where"], lv["spre"], e, P["disc.rn.cond.w:e"],
                                        own_sample=mutate == "where_prior_reads_own_sample").sum(-1) * dpres
    else:
        mean = torch.tensor(cfg.where_prior_mean, dtype=dt)
        dp_where = O.normal_log_prob(lv["d.where"], mean, torch.ones(4, dtype=dt)).sum(-1) * dpres
    if cfg.disc_prior_type == "geom":
        pr = torch.tensor(1.0 - cfg.step_success_prob, dtype=dt)
        p_num = n * torch.log1p(-pr) + torch.log(pr)
        p_num_abs = (n * torch.log1p(-pr)).abs() + torch.log(pr).abs()
    else:
        logits = P["disc.step_prior_bias"] + c["later"].to(dt)[..., None] * P["disc.step_prior_timestep_bias"]
        logits = O.elu(logits + O.mlp_1hidden_out(P, "disc.steps_prior", e))
        p_num = torch.log_softmax(logits, -1).gather(-1, n.long().unsqueeze(-1)).squeeze(-1)
        p_num_abs = logits.gather(-1, n.long().unsqueeze(-1)).squeeze(-1).abs() + torch.logsumexp(logits, -1).abs()
    out.update(disc_what_log_prob=dq_what, disc_where_log_prob=dq_where, disc_what_prior_log_prob=dp_what,
               disc_where_prior_log_prob=dp_where, disc_pres=dpres, disc_prob=joint, disc_log_prob=q_num, disc_prior_log_prob=p_num,
               num_disc_steps_per_sample=n)
    q_terms = [out["prop_what_log_prob"], out["prop_where_log_prob"], q_pres * pres_tm1, dq_what, dq_where, q_num[..., None]]
    p_terms = [out["prop_what_prior_log_prob"], out["prop_where_prior_log_prob"], p_pres * pres_tm1, dp_what, dp_where, p_num[..., None]]
    d_terms = [q_pres * pres_tm1, q_num[..., None]]
    for name, terms in (("qz", q_terms), ("pz", p_terms), ("disc_lp", d_terms)):
        out[name] = sum(t.sum(-1) for t in terms)
        out["abs:" + name] = sum(t.detach().abs().sum(-1) for t in terms)
    out["step_log_prob"] = out["discrete_log_prob"] = out["disc_lp"]
    out["abs:step_log_prob"] = out["abs:discrete_log_prob"] = out["abs:disc_lp"]
    # the per-row scalars: the propagation Bernoulli sums over their slots; the number-of-steps terms over their own two parts
    out["abs:prop_log_prob"] = (q_pres * pres_tm1).detach().abs().sum(-1)
    out["abs:prop_prior_log_prob"] = (p_pres * pres_tm1).detach().abs().sum(-1)
    out["abs:disc_log_prob"] = q_num.detach().abs()
    out["abs:disc_prior_log_prob"] = p_num_abs.detach()
    return out


def evaluate(tape, L, cfg, dtype, mutate=None):
    """The forward outputs as float64 numpy arrays."""
    lv, c = make_leaves(tape, L, cfg, dtype, mutate)
    with torch.no_grad():
        return {k: v.double().numpy() for k, v in forward(lv, c, mutate).items()}


def objective(out, g_lw, g_dl):
    return g_lw * (out["pz"] - out["qz"]) + g_dl * out["disc_lp"]


def adjoint(tape, L, cfg, up, dtype, mutate=None, with_abs=False):
    """up: g_lw, g_dl [T, R].  Returns {leaf name: gradient} (numpy, the leaf's shape; zeros where nothing arrives) for every leaf of
    make_leaves, 'ps' over the used columns, 'm.*' and 'spre' as zeros where the configuration has no such leaf; with_abs (float64):
    also 'abs:P:<name>', per small parameter the sum over (frame, row) of the absolute value of that pair's contribution."""
    lv, c = make_leaves(tape, L, cfg, dtype, mutate)
    out = forward(lv, c, mutate)
    obj = objective(out, _T(up["g_lw"], dtype), _T(up["g_dl"], dtype))
    tot = None
    if with_abs:   # (before the graph is released: one backward pass per (frame, row))
        names = ["P:" + n for n in used_params(cfg)]
        tot = {k: np.zeros(tuple(lv[k].shape)) for k in names}
        flat = obj.reshape(-1)
        for i in range(flat.shape[0]):
            gi = torch.autograd.grad(flat[i], [lv[k] for k in names], retain_graph=True, allow_unused=True)
            for k, v in zip(names, gi):
                if v is not None:
                    tot[k] += v.detach().abs().double().numpy()
    g = adjoints(dict(obj=obj), dict(obj=torch.ones_like(obj)), lv)
    nw = c["nw"]
    for f in Z_FIELDS:
        g.setdefault("m." + f, torch.zeros(field(tape["rec_m"][:obj.shape[0]], L, f, nw).shape, dtype=dtype))
    g.setdefault("spre", torch.zeros(tape["spre"].shape, dtype=dtype))
    for name in SMALL_PARAMS:
        g.setdefault("P:" + name, torch.zeros(np.asarray(tape["params"][name]).shape, dtype=dtype))
    if mutate == "cholesky_swapped":
        g["P:prop.cholesky_scale"] = g["P:prop.cholesky_scale"][[0, 1, 2, 3, 5, 4, 6, 7, 8, 9]]
    if mutate == "absent_e_path_dropped":
        g["m.logit"] = g["m.logit"] * c["m_pres"]
    res = {k: v.double().numpy() for k, v in g.items()}
    if with_abs:
        for name in SMALL_PARAMS:
            res["abs:P:" + name] = tot.get("P:" + name, np.zeros(res["P:" + name].shape))
    return res
