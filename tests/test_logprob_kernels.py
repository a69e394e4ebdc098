"""-m gpu: k_logprob and its adjoint k_logprob_bwd, each on its own against float64.

The two kernels run through their unit entries (sqair_logprob_test, sqair_logprob_bwd_test: the launchers of the forward pass and of
sqair_backward on caller-owned buffers) and are compared with tests/logprob_ref.py -- k_logprob restated on the oracle's functions,
differentiated by autograd, pinned on the CPU by tests/test_logprob_ref.py, which also holds the power check over THIS module's case
list (CASES / build_case are imported there: building a case needs no GPU).

Inputs.  The tape is drawn in float64, rounded to float32, and given as the same float32 values to kernel and reference.  Upstream
gradients g_lw / g_dl are N(0, 1) x 10^U(-2, 1) with exact zeros.  What a kernel must not read is NaN (record fields outside its
contract, rec_m beyond the z segment and its frame T, pitch padding and guard rows of pstats, every parameter but the ones the
configuration uses); what it must not write holds distinct words and is compared bit for bit afterwards (gradient-record columns
outside the seven fields, d_rec_m's frame T, flat_grad outside the segments in use, the frames around t = 2 of the forward's
outputs); accumulated outputs start from known content of mixed magnitude.  Half the cases have a pstats pitch above the width.

Regimes: T = 3, R = 6 (B 3 x K 2) or 5 (B 1 x K 5) rows.  Discovery presence is a prefix of every length 0 .. N; pres_tm1 is
arbitrary (holes), pres <= pres_tm1; (frame 0, row 0) has nothing present anywhere, (frame 1, row 1) everything.  Samples lie up to
4 scales from their locations (75 % of the prior terms too, by construction of the prior location), posterior scales from the floor
1e-2 to 10, raw prior scales from -12 to 3, presence logits within +-12, parameters N(0, 1) x 0.5.  Two draws are conditioned, on the
draw alone: prop.cholesky_scale is redrawn until the factor's diagonal 1 + T_ii is at least 0.3 (a singular factor has no gradient
to compare), and a row's discovery logits until the REFERENCE's joint[n] is at least 1e-12 (asserted per case).  Below the 1e-16
clip of NumStepsDistribution the oracle's straight-through gradient and the kernel's differ by design, and sampling cannot get
there; that regime is not tested.  Nothing is selected on a kernel's result, and no row is left out of a comparison.

Metric and bars.  An element's error is divided by the largest reference magnitude of its row (a where quadruple, the n_what
entries, the N slots of a per-slot scalar, a pstats row, the 128 units of spre); for reduced quantities (qz, pz, disc_lp, the
per-row scalars, every flat_grad entry) by the float64 sum of the absolute terms, per (frame, row) from the reference (plus the
content an accumulated entry starts from).  The bar of a (kernel, output) is 8 x the worst error of the SAME reference in float32
over that kernel's cases.  Presences and step counts are exact.  With SQAIR_PARITY_DIR set the figures go to logprob_parity.json
there (profiles/logprob_parity.json is such a file)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from tests import kernel_unit as U
from tests import logprob_ref as LR
from tests import slot_adjoint_ref as R
from tests.hip_util import stream
from tests.kernel_unit import F32, F64, Buf
from tests.kernel_unit import f32 as _f32, mixed as _mixed

pytestmark = pytest.mark.gpu

HW, T_FRAMES, OUT_T0, OUT_FRAMES = (50, 50), 3, 2, 6           # the forward's outputs: frames 2 .. 4 of tensors 6 frames tall
JOINT_MIN = 1e-12
FLAG_COMBOS = list(itertools.product(("rnn", "rw", "guided"), (True, False), ("cat", "geom")))
TIMES = ("g0", "g5", "rows")        # t_global0 = 0 | t_global0 = 5 | per-row counters (zeros and positives), t_global0 = 7 to be ignored


def _case(wide, N, nw, n_units, rows, combo, time, pitch, outs, seed, **flags):
    ptype, rec_where, dprior = combo
    B, K = (3, 2) if rows == 6 else (1, 5)
    return dict(wide=wide, N=N, nw=nw, n_units=n_units, B=B, K=K, time=time, pitch=pitch, outs=outs, seed=seed,
                flags=dict(flags, prop_prior_type=ptype, rec_where_prior=rec_where, disc_prior_type=dprior))


CASES = {}
for _i, (_N, _nw) in enumerate(itertools.product((1, 3, 4, 5, 8), (1, 7, 50))):
    if (_N, _nw) == (3, 7):
        continue                                                   # (the twelve flag cases below are at this shape)
    _c = FLAG_COMBOS[(5 * _i) % 12]
    CASES["N%d nw%d nu%d %s" % (_N, _nw, 4 if _i % 2 else 8, "-".join(map(str, _c)))] = _case(
        False, _N, _nw, 4 if _i % 2 else 8, 6 if _i % 4 < 2 else 5, _c, TIMES[_i % 3], _i % 2, "all" if _i % 3 else "some", 100 + _i)
for _i, _c in enumerate(FLAG_COMBOS):
    CASES["flags N3 nw7 " + "-".join(map(str, _c))] = _case(False, 3, 7, 8, 6 if _i % 2 else 5, _c, TIMES[(_i + 1) % 3], (_i // 2) % 2,
                                                             "all", 200 + _i)
CASES["flags N3 nw7 off-default guided-False-geom"] = _case(False, 3, 7, 8, 6, ("guided", False, "geom"), "g0", 1, "all", 220,
                                                            prop_prior_step_bias=-1.5, scale_prior="0.5,-1.0", step_success_prob=0.4)
CASES["flags N3 nw7 off-default rnn-True-cat"] = _case(False, 3, 7, 8, 5, ("rnn", True, "cat"), "rows", 0, "some", 221,
                                                       prop_prior_step_bias=2.5)
for _i, (_N, _nw, _nu, _c) in enumerate([(3, 64, 16, ("rnn", True, "cat")), (3, 65, 8, ("guided", True, "cat")),
                                          (3, 128, 8, ("rw", False, "geom")), (9, 50, 8, ("rw", True, "cat")),
                                          (14, 51, 8, ("guided", True, "cat"))]):
    CASES["wide N%d nw%d nu%d %s" % (_N, _nw, _nu, "-".join(map(str, _c)))] = _case(True, _N, _nw, _nu, 5 if _N == 14 else 6, _c,
                                                                                     TIMES[(_i + 2) % 3], (_i + 1) % 2, "all", 300 + _i)


# ------------------------------------------------------------------------------------------------ handles
class _Handle(U.Handle):
    """The handle of a case, with the oracle's configuration and the small parameters' segments of the flat buffer."""

    def __init__(self, case):
        c = CASES[case]
        U.Handle.__init__(self, case, c["wide"], HW, c["N"], c["K"], dict(c["flags"], n_what=c["nw"], n_units=c["n_units"]))
        self.ocfg = O.make_cfg(self.F, HW)
        assert self.nw == c["nw"] and self.nh == 32 * c["n_units"]
        self.seg = {}                  # small parameter -> (first word in flat, shape)
        for name in LR.SMALL_PARAMS:
            if name.endswith(":e"):    # the expected-steps row of disc.rn.cond.w [4 + n_hidden + 1, 128]
                o, n = self.off["disc.rn.cond.w"]
                assert n == (4 + self.nh + 1) * 128 and self.shapes["disc.rn.cond.w"] == (4 + self.nh + 1, 128)
                self.seg[name] = (o + (4 + self.nh) * 128, (128,))
            else:
                o, n = self.off[name]
                assert n == int(np.prod(self.shapes[name]))
                self.seg[name] = (o, self.shapes[name])


def handle(case):
    return U.handle(case, _Handle)


close_handles = U.close
PARITY = U.Parity("logprob_parity.json",
                  "per case of tests/test_logprob_kernels.py and output: the kernel's largest scaled error against the float64 "
                  "reference, the bar (8 x the worst error of the same reference in float32 over the kernel's cases), the float32 "
                  "reference's own error in this case; `bars`: per kernel and output the float32 figure the bar comes from; "
                  "`worst_ratio`: per kernel the largest err / bar", worst_ratio=True)


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    close_handles()
    PARITY.write(worst32)


# ------------------------------------------------------------------------------------------------ the cases (no GPU needed)
def _put(rec, L, name, nw, v):
    c, w = L[LR.COLS.get(name, name)], LR.width(L, name, nw)
    rec[..., c:c + w] = np.asarray(v).reshape(rec.shape[:-1] + (w,))


def _scales(rng, shape):
    """Posterior scales from the floor 1e-2 to 10, both ends occurring exactly."""
    s = 10.0 ** rng.uniform(-2, 1, size=shape)
    u = rng.uniform(size=shape)
    s[u < 0.10] = 1e-2
    s[u > 0.95] = 10.0
    return s


def _z(rng, shape):
    """Standardised distances of a sample from its location: up to 4 scales."""
    return np.clip(rng.standard_normal(shape) * 1.5, -4.0, 4.0)


def _draw_cholesky(rng):
    """prop.cholesky_scale ~ N(0, 1) x 0.5, redrawn until every diagonal entry 1 + T_ii of the factor is at least 0.3."""
    for _ in range(1000):
        v = rng.standard_normal(10) * 0.5
        if np.diagonal(O.fill_triangular(torch.as_tensor(v), 4).numpy()).min() + 1.0 >= 0.3:
            return _f32(v)
    raise AssertionError("no well-conditioned Cholesky factor drawn")


def _draw_prob(rng, n, N):
    """Discovery presence probabilities of one row whose presence is the prefix of length n: logits within +-12, redrawn until the
    reference's joint[n] (float64, from the float32 probabilities) is at least JOINT_MIN."""
    for _ in range(1000):
        lg = rng.uniform(-12, 12, size=N)
        lg[:n] = np.clip(rng.normal(2.5, 3.0, size=n), -12, 12)
        if n < N:
            lg[n] = np.clip(rng.normal(-2.5, 3.0), -12, 12)
        p = _f32(torch.sigmoid(torch.as_tensor(lg)).numpy())
        joint = O.bernoulli_to_modified_geometric(torch.as_tensor(p, dtype=torch.float64)).numpy()
        if joint[n] >= JOINT_MIN and 0.0 < p.min() and p.max() < 1.0:
            return p
    raise AssertionError("no admissible presence probabilities drawn")


def draw_tape(case):
    c = CASES[case]
    hd = handle(case)
    L, N, nw, cfg = hd.L, hd.N, hd.nw, hd.ocfg
    T_, R_ = T_FRAMES, c["B"] * c["K"]
    W, pw = L["W"], 9 + 2 * nw
    rng = np.random.default_rng(5000 + c["seed"])
    ptype = cfg.prop_prior_type
    params = {}
    for name in LR.SMALL_PARAMS:
        params[name] = _draw_cholesky(rng) if name == "prop.cholesky_scale" else _f32(rng.standard_normal(hd.seg[name][1]) * 0.5)
    # presence: discovery a prefix of every length 0 .. N; previous presence arbitrary; propagated <= previous
    assert T_ * R_ >= N + 1
    ns = rng.permutation(np.arange(T_ * R_) % (N + 1)).reshape(T_, R_)
    for (f, r), want in (((0, 0), 0), ((1, 1), N)):                  # the row with nothing / everything present
        at = tuple(np.argwhere(ns == want)[0])
        ns[at], ns[f, r] = ns[f, r], want
    assert set(ns.reshape(-1)) == set(range(N + 1))
    d_pres = (np.arange(N)[None, None, :] < ns[..., None]).astype(F64)
    m_pres = (rng.uniform(size=(T_ + 1, R_, N)) < 0.6).astype(F64)
    p_pres = m_pres[:T_] * (rng.uniform(size=(T_, R_, N)) < 0.7)
    m_pres[0, 0], p_pres[0, 0] = 0.0, 0.0
    m_pres[1, 1], p_pres[1, 1] = 1.0, 1.0
    assert np.all(p_pres <= m_pres[:T_])
    rec_p, rec_d, rec_m = (np.full(s, np.nan) for s in ((T_, R_, N, W), (T_, R_, N, W), (T_ + 1, R_, N, W)))
    sh = (T_, R_, N)
    # posteriors and their samples
    x = {}
    for rec, ph in ((rec_p, "p"), (rec_d, "d")):
        for f in ("where", "what"):
            w = LR.width(L, f, nw)
            loc, sc, z = rng.standard_normal(sh + (w,)), _scales(rng, sh + (w,)), _z(rng, sh + (w,))
            loc, sc = _f32(loc).astype(F64), _f32(sc).astype(F64)
            if ph == "p" and f == "where":   # MultivariateNormalTriL: where = loc + L z, L = T * scale[:, None] + diag(scale)
                Lm = R.where_tril(torch.as_tensor(params["prop.cholesky_scale"], dtype=torch.float64), torch.as_tensor(sc))
                smp = loc + (Lm @ torch.as_tensor(z).unsqueeze(-1)).squeeze(-1).numpy()
            else:
                smp = loc + sc * z
            x[ph + f] = _f32(smp).astype(F64)
            _put(rec, L, f, nw, smp); _put(rec, L, f + "_loc", nw, loc); _put(rec, L, f + "_scale", nw, sc)
    _put(rec_p, L, "PRES", nw, p_pres); _put(rec_d, L, "PRES", nw, d_pres); _put(rec_m, L, "PRES", nw, m_pres)
    _put(rec_p, L, "logit", nw, rng.uniform(-12, 12, size=sh))
    _put(rec_d, L, "PROB", nw, np.stack([[_draw_prob(rng, int(ns[f, r]), N) for r in range(R_)] for f in range(T_)]))
    # the propagation prior: raw scales -12 .. 3 (the floor exactly in a tenth); three quarters of the locations put the sample
    # within 4 prior scales, the rest are free draws
    pstats = np.full((T_, R_, N, pw), np.nan)
    pstats[..., 0] = rng.standard_normal(sh) * 2.0
    raw = rng.uniform(-12, 3, size=sh + (4 + nw,))
    raw[rng.uniform(size=raw.shape) < 0.1] = -12.0
    raw = _f32(raw).astype(F64)
    pstats[..., 5 + nw:] = raw
    psc = (O.softplus(torch.as_tensor(raw)) + 1e-2).numpy()
    want_loc = np.concatenate([x["pwhere"], x["pwhat"]], -1) - psc * _z(rng, raw.shape)
    free = rng.uniform(size=raw.shape) < 0.25
    want_loc[free] = rng.standard_normal(int(free.sum()))
    m_zl = rng.standard_normal((T_ + 1, R_, N, 4 + nw))                          # [where | what] of the previous frame's merged records
    if ptype == "rnn":
        pstats[..., 1:5 + nw] = want_loc
    elif ptype == "rw":
        m_zl[:T_] = want_loc
    else:
        stat = _f32(rng.standard_normal(raw.shape)).astype(F64)
        pstats[..., 1:5 + nw] = stat
        m_zl[:T_] = want_loc - 0.1 * stat
    if ptype != "rnn":
        _put(rec_m, L, "where", nw, m_zl[..., :4]); _put(rec_m, L, "what", nw, m_zl[..., 4:])
        _put(rec_m, L, "logit", nw, rng.uniform(-12, 12, size=(T_ + 1, R_, N)))
    spre = rng.standard_normal((T_, R_, 128)) if cfg.rec_where_prior else np.full((T_, R_, 128), np.nan)
    t_row = np.array([0, 3, 0, 1, 7, 0][:R_], np.int32) if c["time"] == "rows" else None
    t0 = dict(g0=0, g5=5, rows=7)[c["time"]]
    frames = np.arange(T_)[:, None]
    tape = dict(rec_p=_f32(rec_p), rec_d=_f32(rec_d), rec_m=_f32(rec_m), pstats=_f32(pstats), spre=_f32(spre), params=params,
                t=(t0 if t_row is None else t_row[None, :]) + frames + np.zeros((1, R_), np.int64), t_ignored=t0 + frames + np.zeros((1, R_), np.int64))
    up = dict(g_lw=_mixed(rng, (T_, R_)), g_dl=_mixed(rng, (T_, R_)))
    for k in up:
        up[k][rng.uniform(size=(T_, R_)) < 0.15] = 0.0
    up["g_lw"][2, 0] = up["g_dl"][2, 0] = 0.0                                   # a (frame, row) nothing flows into
    return tape, up, dict(t0=t0, t_row=t_row, T=T_, R=R_, pw=pw, ns=ns), rng


def bwd_names(cfg):
    names = ["d_rec_p." + f for f in LR.REC_FIELDS] + ["d_rec_d." + f for f in LR.REC_FIELDS]
    if cfg.prop_prior_type != "rnn":
        names += ["d_rec_m." + f for f in LR.Z_FIELDS]
    return names + ["d_pstats", "d_spre"] + ["flat_grad." + p for p in LR.used_params(cfg)]


def _leaf_of(name):
    kind, _, f = name.partition(".")
    return {"d_rec_p": "p." + f, "d_rec_d": "d." + f, "d_rec_m": "m." + f, "d_pstats": "ps", "d_spre": "spre", "flat_grad": "P:" + f}[kind]


ACCUMULATED = ("d_rec_p", "d_rec_d", "d_rec_m", "flat_grad")


def bwd_outputs(g, content, names, dt):
    """The reference's gradients in the kernel's terms: accumulated outputs include the content they start from (added in `dt`)."""
    out = {}
    for name in names:
        v = np.asarray(g[_leaf_of(name)]).astype(dt)
        if name.split(".")[0] in ACCUMULATED:
            v = content[name].astype(dt) + v
        out[name] = np.asarray(v, F64)
    return out


def fwd_names(outs):
    names = list(LR.REDUCED) + list(LR.PER_ROW) + list(LR.PER_SLOT) + ["disc_prob"]
    if outs == "some":                                                            # every other optional output absent
        names = list(LR.REDUCED) + [n for i, n in enumerate(names[3:]) if i % 2 == 0]
    return names


def fwd_scales(ref, names):
    return {n: ref["abs:" + n] for n in names if "abs:" + n in ref}


def errors(got, ref, scales):
    return {k: R.row_scaled_error(got[k], ref[k], scales.get(k)) for k in ref}


def build_case(case):
    c = CASES[case]
    hd = handle(case)
    cfg, L = hd.ocfg, hd.L
    tape, up, info, rng = draw_tape(case)
    names = bwd_names(cfg)
    content = {}
    for name in names:
        if name.split(".")[0] in ACCUMULATED:
            leaf_name = _leaf_of(name)
            shape = hd.seg[leaf_name[2:]][1] if leaf_name.startswith("P:") else LR.field(tape["rec_p"], L, leaf_name[2:], hd.nw).shape
            content[name] = _mixed(rng, shape, -3.0, 1.0)
    g64 = LR.adjoint(tape, L, cfg, up, torch.float64, with_abs=True)
    g32 = LR.adjoint(tape, L, cfg, up, torch.float32)
    ref = bwd_outputs(g64, content, names, F64)
    scales = {n: g64["abs:P:" + n[len("flat_grad."):]] + np.abs(content[n].astype(F64)) for n in names if n.startswith("flat_grad.")}
    f64, f32 = LR.evaluate(tape, L, cfg, torch.float64), LR.evaluate(tape, L, cfg, torch.float32)
    # the condition of the number-of-steps comparison, on the reference alone
    joint_n = np.take_along_axis(f64["disc_prob"], info["ns"][..., None], -1)[..., 0]
    assert joint_n.min() >= JOINT_MIN * (1 - 1e-6), (case, joint_n.min())
    fn = fwd_names(c["outs"])
    fref = {k: f64[k] for k in fn}
    fsc = fwd_scales(f64, fn)
    return dict(tape=tape, up=up, info=info, content=content, names=names, ref=ref, scales=scales,
                err32=errors(bwd_outputs(g32, content, names, F32), ref, scales), fwd_names=fn, fwd_ref=fref, fwd_scales=fsc,
                fwd_exact={k: f64[k] for k in LR.EXACT}, fwd_err32=errors({k: f32[k] for k in fn}, fref, fsc), joint_min=float(joint_n.min()))


_cases = U.Cases(lambda _: {k: build_case(k) for k in CASES})


def cases():
    return _cases("all")


def worst32(kernel):
    """Per output: the worst error of the fp32 reference over all cases of the kernel."""
    return U.worst32(cases(), "err32" if kernel == "logprob_bwd" else "fwd_err32")


def mutated_errors(case, mutate):
    """(kernel, output) -> error of the float32 reference with the mistake `mutate` in it, in this case and the test's own metric."""
    c, hd = cases()[case], handle(case)
    g = LR.adjoint(c["tape"], hd.L, hd.ocfg, c["up"], torch.float32, mutate=mutate)
    f = LR.evaluate(c["tape"], hd.L, hd.ocfg, torch.float32, mutate=mutate)
    e = {("logprob_bwd", k): v for k, v in errors(bwd_outputs(g, c["content"], c["names"], F32), c["ref"], c["scales"]).items()}
    e.update({("logprob", k): v for k, v in errors({k: f[k] for k in c["fwd_names"]}, c["fwd_ref"], c["fwd_scales"]).items()})
    return e


# ------------------------------------------------------------------------------------------------ on the GPU
def _inputs(case, c, hd):
    """The device inputs both kernels share: records (rec_m's frame T NaN), pstats at its pitch inside guard rows, spre, the
    parameters (NaN but the ones in use), the per-row counters."""
    info, tape, cs = c["info"], c["tape"], CASES[case]
    rec_m = tape["rec_m"].copy()
    rec_m[info["T"]] = np.nan
    ld = info["pw"] + (3 if cs["pitch"] else 0)
    ps = R.Pitched(info["T"] * info["R"] * hd.N, info["pw"], ld, data=tape["pstats"].reshape(-1, info["pw"]))
    flat = np.full(hd.L["n_flat"], np.nan, F32)
    for name in LR.used_params(hd.ocfg):
        o, shape = hd.seg[name]
        flat[o:o + int(np.prod(shape))] = tape["params"][name].reshape(-1)
    B = dict(rec_p=Buf(tape["rec_p"]), rec_d=Buf(tape["rec_d"]), rec_m=Buf(rec_m), pstats=Buf(ps.host), spre=Buf(tape["spre"]), flat=Buf(flat))
    if info["t_row"] is not None:
        B["t_row"] = Buf(info["t_row"])
    return B, ps, ld


def _finish(kernel, case, got, ref, scales, err32, worst):
    assert set(got) == set(ref)                                                            # (row_scaled_error: every row is compared)
    U.judge(PARITY, kernel, case, got, lambda k: R.row_scaled_error(got[k], ref[k], scales.get(k)), err32, worst)


@pytest.mark.parametrize("case", sorted(CASES))
def test_logprob_bwd(case):
    c, hd = cases()[case], handle(case)
    L, N, nw, info = hd.L, hd.N, hd.nw, c["info"]
    T_, R_, W = info["T"], info["R"], L["W"]
    B, ps, ld = _inputs(case, c, hd)
    at = 0
    grads = {}
    for kind, frames in (("d_rec_p", T_), ("d_rec_d", T_), ("d_rec_m", T_ + 1)):
        host = R.distinct_words(frames * R_ * N * W, at).reshape(frames, R_, N, W).copy(); at += host.size
        own = np.zeros(host.shape, bool)
        for name in c["names"]:
            if name.startswith(kind + "."):
                f = name.split(".")[1]
                col, w = L[LR.COLS[f]], LR.width(L, f, nw)
                host[:T_, :, :, col:col + w] = c["content"][name].reshape(T_, R_, N, w)
                own[:T_, :, :, col:col + w] = True
        grads[kind] = B[kind] = Buf(host, own)
    dps = R.Pitched(T_ * R_ * N, ld, ld, nan=False, start=at); at += dps.host.size      # written over the whole pitch
    own = np.zeros(dps.host.shape, bool); own[1:-1] = True
    B["d_pstats"] = Buf(dps.host, own)
    dsp = R.Pitched(T_ * R_, 128, 128, nan=False, start=at); at += dsp.host.size
    own = np.zeros(dsp.host.shape, bool); own[1:-1] = True
    B["d_spre"] = Buf(dsp.host, own)
    fg = R.distinct_words(L["n_flat"], at).copy()
    own = np.zeros(fg.shape, bool)
    for name in c["names"]:
        if name.startswith("flat_grad."):
            o, shape = hd.seg[name[len("flat_grad."):]]
            fg[o:o + int(np.prod(shape))] = c["content"][name].reshape(-1)
            own[o:o + int(np.prod(shape))] = True
    B["flat_grad"] = Buf(fg, own)
    B["g_lw"], B["g_dl"] = Buf(c["up"]["g_lw"]), Buf(c["up"]["g_dl"])
    t = _capi.SqairLogprobBwdTest()
    t.B, t.T, t.t_global0, t.ps_ld = CASES[case]["B"], T_, info["t0"], ld
    t.t_row = B["t_row"].ptr() if "t_row" in B else None
    t.rec_p, t.rec_d, t.rec_m, t.pstats, t.spre = B["rec_p"].ptr(), B["rec_d"].ptr(), B["rec_m"].ptr(), B["pstats"].ptr(ps.first_word()), B["spre"].ptr()
    t.g_lw, t.g_dl, t.flat, t.flat_grad = B["g_lw"].ptr(), B["g_dl"].ptr(), B["flat"].ptr(), B["flat_grad"].ptr()
    t.d_rec_p, t.d_rec_d, t.d_rec_m = B["d_rec_p"].ptr(), B["d_rec_d"].ptr(), B["d_rec_m"].ptr()
    t.d_pstats, t.d_spre = B["d_pstats"].ptr(dps.first_word()), B["d_spre"].ptr(dsp.first_word())
    hd.check(hd.lib.sqair_logprob_bwd_test(hd.h, C.byref(t), stream()), "sqair_logprob_bwd_test")
    for name, b in B.items():
        b.check_untouched(name)
    got = {}
    after = {k: b.after() for k, b in grads.items()}
    d_ps = dps.view(B["d_pstats"].after())
    assert not d_ps[:, info["pw"]:].any(), "d_pstats: the pitch padding is not zeros"
    if not hd.ocfg.rec_where_prior:
        assert not dsp.view(B["d_spre"].after()).any(), "d_spre: not zeros without the recurrent where prior"
    for name in c["names"]:
        kind, _, f = name.partition(".")
        if kind in after:
            got[name] = LR.field(after[kind][:T_], L, f, nw)
        elif kind == "flat_grad":
            o, shape = hd.seg[f]
            got[name] = B["flat_grad"].after()[o:o + int(np.prod(shape))].reshape(shape)
    got["d_pstats"] = d_ps[:, :info["pw"]].reshape(T_, R_, N, info["pw"])
    got["d_spre"] = dsp.view(B["d_spre"].after()).reshape(T_, R_, 128)
    _finish("logprob_bwd", case, got, c["ref"], c["scales"], c["err32"], worst32("logprob_bwd"))


OUT_SHAPE = dict(disc_prob=lambda N: N + 1)


@pytest.mark.parametrize("case", sorted(CASES))
def test_logprob(case):
    c, hd = cases()[case], handle(case)
    N, info = hd.N, c["info"]
    T_, R_ = info["T"], info["R"]
    B, ps, ld = _inputs(case, c, hd)
    at = 0
    red = {}
    for k in LR.REDUCED:                                                          # [T][R] inside guard rows
        red[k] = R.Pitched(T_, R_, R_, nan=False, start=at); at += red[k].host.size
        own = np.zeros(red[k].host.shape, bool); own[1:-1] = True
        B[k] = Buf(red[k].host, own)
    out = _capi.SqairOutputs()
    wanted = [k for k in c["fwd_names"] if k not in LR.REDUCED] + list(LR.EXACT)
    for k in wanted:                                                              # frames OUT_T0 .. OUT_T0 + T of taller tensors
        tail = (N,) if k in LR.PER_SLOT or k in ("prop_pres", "disc_pres") else ((N + 1,) if k == "disc_prob" else ())
        host = R.distinct_words(OUT_FRAMES * R_ * int(np.prod(tail, dtype=int)), at).reshape((OUT_FRAMES, R_) + tail).copy(); at += host.size
        own = np.zeros(host.shape, bool); own[OUT_T0:OUT_T0 + T_] = True
        B["out." + k] = Buf(host, own)
        setattr(out, k, B["out." + k].ptr())
    t = _capi.SqairLogprobTest()
    t.B, t.T, t.t, t.t_global, t.ps_ld = CASES[case]["B"], T_, OUT_T0, info["t0"], ld
    t.t_row = B["t_row"].ptr() if "t_row" in B else None
    t.rec_p, t.rec_d, t.rec_prev, t.pstats, t.spre = B["rec_p"].ptr(), B["rec_d"].ptr(), B["rec_m"].ptr(), B["pstats"].ptr(ps.first_word()), B["spre"].ptr()
    t.flat, t.qz, t.pz, t.disc_lp = B["flat"].ptr(), B["qz"].ptr(red["qz"].first_word()), B["pz"].ptr(red["pz"].first_word()), B["disc_lp"].ptr(red["disc_lp"].first_word())
    t.out = C.addressof(out)
    hd.check(hd.lib.sqair_logprob_test(hd.h, C.byref(t), stream()), "sqair_logprob_test")
    for name, b in B.items():
        b.check_untouched(name)
    got = {k: red[k].view(B[k].after()) for k in LR.REDUCED}
    for k in wanted:
        got[k] = B["out." + k].after()[OUT_T0:OUT_T0 + T_]
    for k in LR.EXACT:
        assert np.array_equal(got.pop(k).astype(F64), c["fwd_exact"][k]), k + " is not exact"
    _finish("logprob", case, got, c["fwd_ref"], c["fwd_scales"], c["fwd_err32"], worst32("logprob"))
