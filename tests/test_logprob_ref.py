"""The float64 reference of the log-probability kernels (tests/logprob_ref.py), pinned without a GPU: its forward reproduces
SqairOracle.timestep for all twelve (prior type x where prior x step prior) combinations at t = 0 and t > 0 from a tape cut out of
the oracle's own outputs, autograd agrees with central differences, the Cholesky gradient lands where oracle.fill_triangular says --
and the power check: every mistake of logprob_ref.MUTATIONS, applied to the float32 evaluation, is seen by at least one (case,
output) of the GPU test's own case list at that output's bar."""
import contextlib
import itertools

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd.flags import make_flags
from sqair_amd.params import init_params
from tests import logprob_ref as LR
from tests import slot_adjoint_ref as R

F64 = torch.float64
HW, G, NW, NH, N, B = (12, 13), 5, 7, 128, 3, 6
# a record layout of this test's own: the reference takes the columns from whatever layout it is given
L = dict(W=40, WHERE=1, WHAT=5, PRES=12, LOGIT=13, WHERE_LOC=14, WHERE_SCALE=18, WHAT_LOC=22, WHAT_SCALE=29, PROB=36)
COMBOS = list(itertools.product(("rnn", "rw", "guided"), (True, False), ("cat", "geom")))


@contextlib.contextmanager
def recorded():
    """Every call of oracle.linear (its output), by layer name, in call order."""
    rec = {}
    lin = O.linear

    def linear(P, name, x):
        y = lin(P, name, x)
        rec.setdefault(name, []).append(y)
        return y
    O.linear = linear
    try:
        yield rec
    finally:
        O.linear = lin


def oracle_tape(ptype, rec_where, dtype_prior, t, seed=0):
    """One SqairOracle.timestep on a small model and the tape of it in the kernels' terms (one frame: T = 1, R = B)."""
    F = make_flags(n_units=NH // 32, n_what=NW, glimpse_size=G, n_steps_per_image=N, k_particles=1, prop_prior_type=ptype,
                   rec_where_prior=rec_where, disc_prior_type=dtype_prior, prop_prior_step_bias=1.5, scale_prior="-1.5,0.5",
                   step_success_prob=0.6)
    P = init_params(F, HW, seed=5 + seed, jitter=0.3)
    P["prop.cholesky_scale"] = np.linspace(-0.6, 0.7, 10)
    cfg = O.make_cfg(F, HW)
    orc = O.SqairOracle(P, cfg, F64)
    rng = np.random.default_rng(17 + seed)
    tn = lambda *s: torch.as_tensor(rng.standard_normal(s))
    pres_tm1 = torch.as_tensor([[1, 1, 0], [0, 0, 0], [1, 0, 1], [1, 1, 1], [0, 1, 0], [1, 0, 0]], dtype=F64)[..., None]
    z_tm1 = (tn(B, N, NW), tn(B, N, 4) * 0.5, pres_tm1, tn(B, N, 1) * 2.0)
    noise = tn(B, 2, N, NW + 5)
    noise[..., -1] = torch.as_tensor(rng.uniform(size=(B, 2, N)))
    with recorded() as rec:
        out = orc.timestep(torch.as_tensor(rng.uniform(size=(B,) + HW)), z_tm1, tn(B, N, NH) * 0.5, tn(B, N, NH) * 0.5,
                           torch.zeros(B, 1, dtype=F64), torch.arange(N, dtype=F64)[None, :, None].expand(B, N, 1), t, noise)

    def records(o):
        r = np.full((1, B, N, L["W"]), np.nan)
        for f, k in (("where", "where"), ("what", "what"), ("logit", "presence_logit"), ("where_loc", "where_loc"),
                     ("where_scale", "where_scale"), ("what_loc", "what_loc"), ("what_scale", "what_scale"), ("PRES", "presence"),
                     ("PROB", "presence_prob")):
            c, w = L[LR.COLS.get(f, f)], LR.width(L, f, NW)
            r[0, :, :, c:c + w] = o[k].detach().numpy().reshape(B, N, w)
        return r
    rec_m = np.full((2, B, N, L["W"]), np.nan)
    for f, v in zip(("what", "where", "PRES", "logit"), z_tm1):
        c, w = L[LR.COLS.get(f, f)], LR.width(L, f, NW)
        rec_m[0, :, :, c:c + w] = v.numpy()
    prior_logit = out["prop"]["prior_stats"][-1].squeeze(-1)
    e = ((torch.sigmoid(prior_logit) - 0.5) / N).sum(-1, keepdim=True)
    cond_w = orc.P["disc.rn.cond.w"]
    params = {k: orc.P[k.split(":")[0]].detach().numpy() for k in LR.SMALL_PARAMS}
    params["disc.rn.cond.w:e"] = cond_w[4 + NH].detach().numpy()
    spre = (rec["disc.rn.cond"][0] - e * cond_w[4 + NH]).detach().numpy()[None] if rec_where else np.full((1, B, 128), np.nan)
    tape = dict(rec_p=records(out["prop"]), rec_d=records(out["disc"]), rec_m=rec_m,
                pstats=rec["prop.prior_linear"][0].detach().numpy().reshape(1, B, N, 9 + 2 * NW), spre=spre,
                t=np.full((1, B), t), params=params)
    return cfg, tape, out


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), b.detach().numpy().reshape(np.shape(a))
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max()), np.abs(a - b).max()


@pytest.mark.parametrize("t", [0, 4])
@pytest.mark.parametrize("ptype,rec_where,dprior", COMBOS)
def test_forward_reproduces_the_oracle_timestep(ptype, rec_where, dprior, t):
    cfg, tape, out = oracle_tape(ptype, rec_where, dprior, t)
    got = LR.evaluate(tape, L, cfg, F64)
    prop, disc = out["prop"], out["disc"]
    assert float(prop["presence"].sum()) > 0 and float(disc["presence"].sum()) > 0
    _close(got["qz"][0], out["q_z_given_x"]); _close(got["pz"][0], out["p_z"]); _close(got["disc_lp"][0], out["presence_log_prob"])
    for k in ("what_log_prob", "where_log_prob", "what_prior_log_prob", "where_prior_log_prob"):
        _close(got["prop_" + k][0], prop[k]); _close(got["disc_" + k][0], disc[k])
    _close(got["prop_prob"][0], prop["prop_prob"]); _close(got["prop_log_prob"][0], prop["prop_log_prob"])
    _close(got["prop_prior_log_prob"][0], prop["prop_prior_log_prob"]); _close(got["disc_prob"][0], disc["num_steps_prob"])
    _close(got["disc_log_prob"][0], disc["num_step_log_prob"]); _close(got["disc_prior_log_prob"][0], disc["num_step_prior_log_prob"])
    _close(got["num_prop_steps_per_sample"][0], prop["num_steps"]); _close(got["num_disc_steps_per_sample"][0], disc["num_steps"])
    # the terms the reduced scalars are judged against add up to at least the scalars
    for k in LR.REDUCED:
        assert np.all(got["abs:" + k] >= np.abs(got[k]) * (1 - 1e-12))


def _ups(rng, shape):
    return dict(g_lw=rng.standard_normal(shape), g_dl=rng.standard_normal(shape))


@pytest.mark.parametrize("ptype,rec_where,dprior", [("guided", True, "cat"), ("rw", False, "geom"), ("rnn", True, "cat")])
def test_autograd_agrees_with_central_differences(ptype, rec_where, dprior):
    cfg, tape, _ = oracle_tape(ptype, rec_where, dprior, 3, seed=1)
    rng = np.random.default_rng(2)
    up = _ups(rng, (1, B))
    g = LR.adjoint(tape, L, cfg, up, F64)

    def value(name, idx, delta):
        lv, c = LR.make_leaves(tape, L, cfg, F64)
        with torch.no_grad():
            lv[name].reshape(-1)[idx] += delta
            return float(LR.objective(LR.forward(lv, c), torch.as_tensor(up["g_lw"]), torch.as_tensor(up["g_dl"])).sum())
    lv0, _ = LR.make_leaves(tape, L, cfg, F64)
    checked = 0
    for name in lv0:
        flat = g[name].reshape(-1)
        for idx in rng.choice(flat.size, size=min(3, flat.size), replace=False):
            h = 1e-5
            fd = (value(name, idx, h) - value(name, idx, -h)) / (2 * h)
            assert abs(fd - flat[idx]) <= 1e-6 * max(1.0, abs(flat[idx])), (name, int(idx), fd, flat[idx])
            checked += 1
    assert checked >= 3 * 15
    # per (frame, row) contributions of the small parameters: their absolute sum bounds the gradient
    ga = LR.adjoint(tape, L, cfg, up, F64, with_abs=True)
    for name in LR.used_params(cfg):
        assert np.all(ga["abs:P:" + name] >= np.abs(ga["P:" + name]) * (1 - 1e-9)), name


def test_cholesky_gradient_lands_where_fill_triangular_says():
    """The gradient of entry v[q] of prop.cholesky_scale is the gradient of the element of the factor that fill_triangular puts v[q]
    in: flat index i * 4 + j of the lower triangle is v[4 + q] for q < 6 and v[15 - q] otherwise."""
    v = torch.arange(10, dtype=F64)
    m = O.fill_triangular(v, 4)
    for i in range(4):
        for j in range(i + 1):
            q = i * 4 + j
            assert int(m[i, j]) == (4 + q if q < 6 else 15 - q)
    cfg, tape, _ = oracle_tape("rnn", False, "geom", 0, seed=2)
    up = _ups(np.random.default_rng(3), (1, B))
    g = LR.adjoint(tape, L, cfg, up, F64)["P:prop.cholesky_scale"]
    # the same gradient through the factor's elements: d obj / d T[i][j], scattered by fill_triangular's own placement
    lv, c = LR.make_leaves(tape, L, cfg, F64)
    Tm = O.fill_triangular(lv["P:prop.cholesky_scale"], 4).detach().requires_grad_(True)
    sc = lv["p.where_scale"]
    Lm = Tm[None] * sc[..., :, None] + torch.diag_embed(sc)
    q_where = O.SqairOracle.mvn_tril_log_prob(lv["p.where"], lv["p.where_loc"], Lm) * c["m_pres"] * c["p_pres"]
    (gT,) = torch.autograd.grad((-torch.as_tensor(up["g_lw"])[..., None] * q_where).sum(), [Tm])
    want = np.zeros(10)
    for i in range(4):
        for j in range(i + 1):
            want[int(m[i, j])] = float(gT[i, j])
    assert np.abs(want).min() > 0 and np.allclose(g, want, rtol=1e-12, atol=0)
    assert len(set(np.round(g, 12))) == 10   # ten different values: a swap of two entries cannot go unnoticed


# ------------------------------------------------------------------------------------------------ the power check
# where each mistake can show at all: the cases tried first (any other case may still catch it)
def _relevant(mutate, case, K):
    c = K.CASES[case]
    ptype, rec_where, cat = c["flags"]["prop_prior_type"], c["flags"]["rec_where_prior"], c["flags"]["disc_prior_type"] == "cat"
    return dict(cholesky_swapped=True, t_row_ignored=c["time"] == "rows" and cat, rec_m_late=True, guided_as_rnn=ptype == "guided",
                stop_term_dropped=True, absent_e_path_dropped=ptype != "rnn" and (rec_where or cat), where_prior_reads_own_sample=rec_where,
                what_column_64_dropped=c["nw"] >= 64)[mutate]


@pytest.fixture(scope="module")
def gpu_cases():
    from tests import test_logprob_kernels as K
    K.cases()
    yield K
    K.close_handles()


def test_gpu_case_list_meets_its_conditions(gpu_cases):
    """What the GPU cases promise about their draws, verified here: the reference's joint[n] stays above the 1e-12 the comparison of
    the number-of-steps terms is conditioned on (far above the 1e-16 clip), every discovery count 0 .. N occurs, a row has nothing
    present and one has everything, previous presence has holes, and the hidden widths are not padded."""
    K = gpu_cases
    shapes = set()
    for name, c in K.cases().items():
        hd, tape = K.handle(name), c["tape"]
        assert c["joint_min"] >= 1e-12 * (1 - 1e-6), (name, c["joint_min"])
        pres = lambda rec: LR.field(rec, hd.L, "PRES", hd.nw)
        p, d, m = pres(tape["rec_p"]), pres(tape["rec_d"]), pres(tape["rec_m"])[:3]
        assert set(d.sum(-1).reshape(-1).astype(int)) == set(range(hd.N + 1)), name
        assert np.all(np.diff(d, axis=-1) <= 0) and np.all(p <= m)
        assert not (p[0, 0].any() or d[0, 0].any() or m[0, 0].any()) and p[1, 1].all() and d[1, 1].all() and m[1, 1].all()
        if hd.N >= 3:
            assert any(row[0] == 0 and row[1:].any() for row in m.reshape(-1, hd.N)), name + ": no hole in pres_tm1"
        shapes.add((K.CASES[name]["wide"], hd.N, hd.nw))
        assert hd.nh in (128, 256, 512)
    assert {(False, n, w) for n in (1, 3, 4, 5, 8) for w in (1, 7, 50)} <= shapes
    assert {(True, 3, 64), (True, 3, 65), (True, 3, 128), (True, 9, 50), (True, 14, 51)} <= shapes


@pytest.mark.parametrize("mutate", LR.MUTATIONS)
def test_gpu_cases_see_the_mistake(gpu_cases, mutate):
    """The mistake, made in the float32 evaluation of the reference, puts at least one (case, output) of the GPU test over that
    output's bar in the GPU test's own metric."""
    K = gpu_cases
    bars = {(kern, k): R.bar_from_fp32(v) for kern in ("logprob", "logprob_bwd") for k, v in K.worst32(kern).items()}
    order = sorted(K.CASES, key=lambda n: (not _relevant(mutate, n, K), n))
    assert _relevant(mutate, order[0], K), "no case where the mistake can show"
    for case in order:
        over = {k: (e, bars[k]) for k, e in K.mutated_errors(case, mutate).items() if not e <= bars[k]}
        if over:
            print(mutate, "seen by", case, {k: "%.2e > %.2e" % v for k, v in over.items()})
            return
    raise AssertionError("no (case, output) of tests/test_logprob_kernels.py exceeds its bar with " + mutate)
