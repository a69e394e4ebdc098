"""-m gpu: the forward kernels of the slot loop, each on its own against a float64 reference.

k_crop_row (generic, not staged, specialised; with the transform's output layer in the launch or without), k_slot_tail<what_done>,
k_rnn_tail<NH, TN, what_done> and k_linear_what<NCH, MODE> run through their unit entries (sqair_slot_crop_test, sqair_slot_tail_test,
sqair_linear_what_test: the pass's own argument builders and launchers on caller-owned buffers) and are compared with
tests/slot_forward_ref.py -- tail_forward / crop_forward of the adjoint reference plus the presence Bernoulli, the z-record, the next
slot's layer and the head layers, on the oracle's functions, pinned on the CPU by tests/test_slot_forward_ref.py.

Inputs are drawn in float64, rounded to float32, and given as the same float32 values to the kernel and to both references.  What the
header's contract says a launch does not read is NaN: the other slots, phases and columns of the input records and of the noise,
pitch padding and guard rows (slot_adjoint_ref.Pitched), every parameter but the rows the launch is about (the packs are made by
sqair_pack_params from such a buffer), enc / hraw / the `what` noise under what_done.  What it does not write holds distinct words
compared bit for bit afterwards: the rest of rec_new (the record the launch writes into starts as distinct words but for the columns
it reads), the frames' padding, the guard rows and padding of out / tp_out / s1h_out.

Metric and bars.  An element's error is divided by the largest magnitude of the reference in its row (slot_adjoint_ref.
row_scaled_error); the bar of a (kernel, output) is bar_from_fp32 of the SAME reference in float32 over that kernel's cases.  Two outputs
take another scale, for a stated reason: the presence LOGIT is a sum of n_hidden / 2 products that may cancel -- an error relative to
the result would make the bar whatever the worst cancellation among the cases is -- so it is judged on the float64 sum of the absolute
terms (previous presence 0: on the 88); the presence PROBABILITY is compared with a uniform on [0, 1) and enters the log-weights as a
probability, so it is judged on the scale 1 (relative to itself it would test how v_rcp_f32 treats the denormal sigmoid(-88)).
k_linear_what's what_loc and what are sums that cancel as well (a product over n_hidden inputs, the gated mixture), and at n_what = 1 a
row has no neighbour to take a scale from: they are judged on the row maximum of their absolute terms too.  Presences are exact, every
row, no exception.

The presence condition.  A row's uniform is placed from the float64 reference alone: |u - prob64| >= 1e-3 (three orders above the
float32 error of a sigmoid at |logit| <= 32), one row of each case has u = 0 and one the largest float below 1; the builder asserts
that the float32 and float64 references then agree on every presence.  Nothing is selected on a kernel's result.

A glimpse wholly outside the frame does not exist under to_coords (the shift is a tanh: the glimpse's centre is inside the frame); the
crop cases put saturated shifts with large scales in their first rows, which leaves most of those glimpses outside.

With SQAIR_PARITY_DIR set the figures go to slot_forward_parity.json there (the copy under profiles/ is such a file)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from tests import kernel_unit as U
from tests import slot_adjoint_ref as R
from tests import slot_forward_ref as SF
from tests.hip_util import dev, stream
from tests.kernel_unit import CHOLESKY, F32, F64, SCALE_OFFSET, Buf, pitched
from tests.kernel_unit import bits as _bits, f32 as _f32, image as _image, records as _sentinel_records

pytestmark = pytest.mark.gpu

T64, T32 = torch.float64, torch.float32
U_MARGIN = 1e-3
U_MAX = float(np.nextafter(F32(1.0), F32(0.0)))

# ------------------------------------------------------------------------------------------------ handles
HANDLES = {   # name: (wide, (H, W), N, K, flags)
    "f_50_256": (False, (50, 50), 4, 1, dict()),
    "f_7_128": (False, (50, 50), 3, 1, dict(n_what=7, n_units=4)),
    "f_1_256": (False, (50, 50), 3, 1, dict(n_what=1)),
    "f_10_128": (False, (50, 50), 3, 1, dict(n_what=10, n_units=4)),
    "f_33_256": (False, (50, 50), 3, 1, dict(n_what=33)),
    "f_3_128": (False, (50, 50), 3, 1, dict(n_what=3, n_units=4)),
    "f_50_128_k17": (False, (50, 50), 2, 17, dict(n_units=4)),
    "f_64_256_wide": (True, (50, 50), 3, 1, dict(n_what=64)),
    "f_65_512_wide": (True, (50, 50), 14, 1, dict(n_what=65, n_units=16)),
    "f_128_256_wide": (True, (50, 50), 3, 1, dict(n_what=128)),
    "k_50x50": (False, (50, 50), 4, 3, dict()),
    "k_37x41_g12": (False, (37, 41), 3, 5, dict(glimpse_size=12)),
    "k_64x64_g28": (False, (64, 64), 8, 2, dict(glimpse_size=28)),
    "k_72x64_128": (False, (72, 64), 1, 3, dict(n_units=4)),
    "k_3x250": (False, (3, 250), 4, 2, dict()),
    "k_257x5_g12": (False, (257, 5), 3, 1, dict(glimpse_size=12)),
    "k_50x50_512_wide": (True, (50, 50), 3, 3, dict(n_units=16)),
}


def handle(name):
    return U.handle(name, lambda n: U.Handle(n, *HANDLES[n]))


close_handles = U.close
PARITY = U.Parity("slot_forward_parity.json",
                  "per case of tests/test_slot_forward_kernels.py and output: the kernel's largest row-scaled error against the float64 "
                  "reference, the bar (8 x the worst error of the same reference in float32 over the kernel's cases), the float32 "
                  "reference's own error in this case; `bars`: per kernel and output the float32 figure the bar comes from")


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    close_handles()
    PARITY.write(worst32)


# ------------------------------------------------------------------------------------------------ errors, bars
def _scaled(name, ref):
    """The scale of an output that is not its row's largest reference magnitude: `<name>_terms` (the float64 absolute terms of the
    sums behind it; their row maximum), 1 for the probability."""
    if name == "prob":
        return np.ones_like(ref["prob"])
    return ref[name + "_terms"].max(-1, keepdims=True) if name + "_terms" in ref else None


def errors(got, ref):
    """Per output of `ref` (the float64 reference, with its scales): the row-scaled error of `got`; presences: 0 if equal, else inf."""
    e = {}
    for k, v in ref.items():
        if k.endswith("_terms"):
            continue
        if k == "pres":
            e[k] = 0.0 if np.array_equal(np.asarray(got[k], F64), v) else float("inf")
        else:
            e[k] = R.row_scaled_error(got[k], v, _scaled(k, ref))
    return e


_cases = U.Cases(lambda kernel: {k: BUILD[kernel](*v) for k, v in CASES[kernel].items()})


def cases(kernel=None):
    return {k: _cases(k) for k in CASES} if kernel is None else _cases(kernel)


def worst32(kernel):
    """Per output: the worst error of the float32 reference over all cases of the kernel."""
    return U.worst32(cases(kernel))


def mutated_errors(kernel, case, mistake):
    """The errors of the float32 reference making `mistake`, in the metric of the test (tests/test_slot_forward_ref.py)."""
    c = cases(kernel)[case]
    with SF.mistake(mistake):
        got = EVAL[kernel](c["inp"], T32)
    return errors(got, c["ref"])


def _finish(kernel, inp):
    ref = EVAL[kernel](inp, T64)
    ref32 = EVAL[kernel](inp, T32)
    err32 = errors(ref32, ref)
    assert err32.get("pres", 0.0) == 0.0, "the float32 and float64 references disagree on a presence"
    return dict(inp=inp, ref=ref, err32=err32)


def _judge(kernel, case, got, c):
    """Every output under its bar (all of them measured and recorded first); presences are exact."""
    e = errors(got, c["ref"])
    U.judge(PARITY, kernel, case, e, e.get, c["err32"], worst32(kernel), exact=("pres",))


# ------------------------------------------------------------------------------------------------ the tail family: inputs
def _gate_raws(rng, shape):
    """A third out to +-20, the others N(0, 1.5)."""
    return np.where(rng.uniform(size=shape) < 0.33, rng.uniform(-20, 20, size=shape), rng.standard_normal(shape) * 1.5)


def _scales(rng, shape):
    """softplus(raw) + 1e-2 with raw in [-12, 10]: from the floor to 10."""
    return (O.softplus(torch.as_tensor(rng.uniform(-12.0, 10.0, size=shape))) + 1e-2).numpy()


def _steps_params(rng, core, nh, nw, shapes):
    """The steps predictor's parameters as the oracle shapes them; of l0.w only the `what` rows are numbers.  w2 is sized for presence
    logits out to +-30."""
    nsp = nh // 2
    w0 = np.full(shapes[core + ".steps.l0.w"], np.nan, F32)
    r0, r1 = SF.rows_of(SF.STEPS_FEATURES[core], "what", nh, nw)
    assert r1 == w0.shape[0] and w0.shape[1] == nsp
    w0[r0:r1] = _f32(rng.standard_normal((nw, nsp)) * 0.4 / np.sqrt(nw))
    return {core + ".steps.l0.w": w0, core + ".steps.l1.w": _f32(rng.standard_normal((nsp, 1)) * 10.0 / np.sqrt(nsp)),
            core + ".steps.l1.b": np.array([0.25], F32)}


def _records_for(hd, R_, is_disc, slot, rng, prev, what_tm1=None, where=None, start=0):
    """rec_prev (NaN but for what the launch reads) and rec_new (distinct words but for what it reads)."""
    L, N, W = hd.L, hd.N, hd.L["W"]
    rec_prev = np.full((R_, N, W), np.nan, F32)
    rec_new = _sentinel_records(R_, N, W, start)
    if is_disc and slot > 0:
        rec_new[:, slot - 1, L["PRES"]] = prev
    if not is_disc:
        rec_prev[:, slot, L["PRES"]] = prev
        if what_tm1 is not None:
            rec_prev[:, slot, L["WHAT"]:L["WHAT"] + hd.nw] = what_tm1
    if where is not None:
        rec_new[:, slot, L["WHERE"]:L["WHERE"] + 4] = where
    return rec_prev, rec_new


def _prev(rng, R_, is_disc, slot):
    prev = (rng.uniform(size=R_) < 0.6).astype(F32)
    prev[0] = 1.0
    if R_ > 1:
        prev[1] = 0.0
    if R_ > 3:
        prev[2:4] = 1.0
    if is_disc and slot == 0:
        prev[:] = 1.0                                   # (taken without a read)
    return prev


def _place_u(prob64, prev, rng):
    """Uniforms at least U_MARGIN from the float64 probability; the first two eligible present rows get u = 0 and the largest float
    below 1."""
    u = rng.uniform(size=prob64.shape)
    near = np.abs(u - prob64) < 2 * U_MARGIN
    u[near] = np.where(prob64[near] < 0.5, prob64[near] + 2 * U_MARGIN, prob64[near] - 2 * U_MARGIN)
    u = u.astype(F32)
    ok0 = np.flatnonzero((prev > 0) & (prob64 >= 2 * U_MARGIN))
    ok1 = np.flatnonzero((prev > 0) & (prob64 <= 1 - 2 * U_MARGIN))
    if len(ok0):
        u[ok0[0]] = 0.0
    ok1 = ok1[ok1 != (ok0[0] if len(ok0) else -1)]
    if len(ok1):
        u[ok1[0]] = U_MAX
    assert np.all(np.abs(u.astype(F64) - prob64) >= U_MARGIN) and np.all((u >= 0) & (u < 1))
    return u


def _take(inp, n):
    """The first n rows of a case's inputs."""
    out = dict(inp)
    for k in inp["row_arrays"]:
        if inp[k] is not None:
            out[k] = inp[k][:n].copy()
    out["R"] = n
    return out


def build_tail(hname, is_disc, slot, R_, wd, s1h, seed, rnn=False, take=None):
    hd = handle(hname)
    nw, nh, nsp, N = hd.nw, hd.nh, hd.nh // 2, hd.N
    core = "disc" if is_disc else "prop"
    rng = np.random.default_rng(5000 + seed)
    P = _steps_params(rng, core, nh, nw, hd.shapes)
    prev = _prev(rng, R_, is_disc, slot)
    enc = _f32(np.concatenate([rng.standard_normal((R_, nw)), _scales(rng, (R_, nw))], -1))
    hraw = what_tm1 = where = hid = add = None
    if not is_disc:
        hraw = _f32(np.concatenate([rng.standard_normal((R_, nw)), rng.uniform(-12, 10, size=(R_, nw)), _gate_raws(rng, (R_, 3 * nw))], -1))
        what_tm1 = _f32(rng.standard_normal((R_, nw)))
    if rnn:
        where = _f32(rng.standard_normal((R_, 4)) * 1.5)
        hid = _f32(np.tanh(rng.standard_normal((R_, nh))))
        add = _f32(rng.standard_normal((R_, nh)) * 1.5)
        Wi = np.full(hd.shapes[core + ".rnn.i2h.w"], np.nan, F32)
        for f in ("what", "where", "pres"):
            r0, r1 = SF.rows_of(SF.RNN_INPUT[core], f, nh, nw)
            Wi[r0:r1] = _f32(rng.standard_normal((r1 - r0, nh)) * 0.5 / np.sqrt(nw + 5))
        P[core + ".rnn.i2h.w"] = Wi
        P[core + ".rnn.h2h.w"] = _f32(rng.standard_normal((nh, nh)) / np.sqrt(nh))
    rec_prev, rec_new = _records_for(hd, R_, is_disc, slot, rng, prev, what_tm1, where)
    noise = np.full((R_, 2, N, hd.nzw), np.nan, F32)
    ph = 1 if is_disc else 0
    noise[:, ph, slot, 4:4 + nw] = _f32(rng.standard_normal((R_, nw)))
    noise[:, ph, slot, 4 + nw] = 0.5
    inp = dict(hname=hname, is_disc=bool(is_disc), slot=slot, R=R_, wd=bool(wd), s1h=bool(s1h), rnn=bool(rnn), P=P, enc=enc, hraw=hraw,
               rec_prev=rec_prev, rec_new=rec_new, noise=noise, s1p=_f32(rng.standard_normal((R_, nsp)) * 1.5), hid=hid, add=add,
               what_given=None, row_arrays=("enc", "hraw", "rec_prev", "rec_new", "noise", "s1p", "hid", "add", "what_given"))
    if take is not None:
        inp = _take(inp, take)
    # the sample (what_done: handed over in rec_new) and the uniforms come from the float64 reference
    first = eval_tail(dict(inp, wd=False), T64)
    L = hd.L
    if wd:
        inp["what_given"] = _f32(first["what"])
        inp["rec_new"][:, slot, L["WHAT"]:L["WHAT"] + nw] = inp["what_given"]
        inp["noise"][:, ph, slot, 4:4 + nw] = np.nan          # not read then
        first = eval_tail(inp, T64)
    inp["noise"][:, ph, slot, 4 + nw] = _place_u(first["prob"][:, 0], inp["rec_prev"][:, slot, L["PRES"]] if not is_disc else
                                                 (np.ones(inp["R"], F32) if slot == 0 else inp["rec_new"][:, slot - 1, L["PRES"]]), rng)
    c = _finish("rnn_tail" if rnn else "slot_tail", inp)
    prev_rows = SF.slot_operands(inp["rec_prev"], inp["rec_new"], inp["noise"], L, is_disc, slot, nw, T64)["prev"].numpy()
    absent = prev_rows == 0
    assert np.all(c["ref"]["logit"][absent, 0] == -88.0) and not c["ref"]["pres"][absent].any()
    return c


def eval_tail(inp, dtype):
    hd = handle(inp["hname"])
    nw, nh, slot, is_disc = hd.nw, hd.nh, inp["slot"], inp["is_disc"]
    core = "disc" if is_disc else "prop"
    P = SF.params(inp["P"], dtype)
    ops = SF.slot_operands(inp["rec_prev"], inp["rec_new"], inp["noise"], hd.L, is_disc, slot, nw, dtype)
    s1p = R.T(inp["s1p"], dtype)
    if inp["wd"]:
        t = SF.tail(P, core, nh, ops, s1p, what=R.T(inp["what_given"], dtype))
    else:
        enc = R.T(inp["enc"], dtype)
        t = SF.tail(P, core, nh, ops, s1p, enc_loc=enc[:, :nw], enc_scale=enc[:, nw:], hraw=None if is_disc else R.T(inp["hraw"], dtype))
    out = dict(logit=t["logit"][:, None], prob=t["prob"][:, None], pres=t["pres"], logit_terms=t["logit_terms"][:, None])
    if not inp["wd"]:
        out.update(what=t["what"], what_loc=t["what_loc"], what_scale=t["what_scale"])
    if inp["s1h"]:
        out["s1h"] = t["hidden"]
    if inp["rnn"]:
        W0 = hd.L["WHERE"]
        z = SF.z_record(R.T(inp["rec_new"], dtype)[:, slot, W0:W0 + 4], t["what"], t["pres"], t["logit"])
        out["out"] = SF.next_slot_layer(P, core, nh, z, R.T(inp["hid"], dtype), R.T(inp["add"], dtype))
    return SF.np64(out)


def run_tail(c, what_done_from=None):
    """One launch of sqair_slot_tail_test on the case's inputs; returns the outputs by name (raw float32 arrays).  what_done_from: a
    rec_new to start from (the what sample written by another launch)."""
    inp = c["inp"]
    hd = handle(inp["hname"])
    L, N, nw, nh, nsp, R_, slot = hd.L, hd.N, hd.nw, hd.nh, hd.nh // 2, inp["R"], inp["slot"]
    wd = inp["wd"] or what_done_from is not None
    flat = Buf(hd.flat_of(inp["P"]))
    packed = hd.pack(flat)
    rec_new0 = inp["rec_new"] if what_done_from is None else what_done_from
    own = np.zeros(rec_new0.shape, bool)
    cols = ["PRES", "LOGIT", "PROB"]
    own[:, slot, [L[k] for k in cols]] = True
    if not wd:
        for k in ("WHAT", "WHAT_LOC", "WHAT_SCALE"):
            own[:, slot, L[k]:L[k] + nw] = True
    B = dict(flat=flat, rec_new=Buf(rec_new0, own), rec_prev=Buf(inp["rec_prev"]), noise=Buf(inp["noise"]))
    t = _capi.SqairSlotTailTest()
    t.is_disc, t.slot, t.B, t.what_done = int(inp["is_disc"]), slot, R_, int(wd)
    t.rec_prev, t.rec_new, t.noise, t.flat, t.packed = B["rec_prev"].ptr(), B["rec_new"].ptr(), B["noise"].ptr(), flat.ptr(), packed
    B["s1p"], t.s1p = pitched(R_, nsp, nsp + 8, inp["s1p"]); t.s1p_ld = nsp + 8
    nan = lambda a: np.full(a.shape, np.nan, F32) if wd else a          # not read under what_done
    B["enc"], t.enc = pitched(R_, 2 * nw, 2 * nw + 5, nan(inp["enc"])); t.enc_ld = 2 * nw + 5
    if not inp["is_disc"]:
        B["hraw"], t.hraw = pitched(R_, 5 * nw, 5 * nw + 3, nan(inp["hraw"])); t.h_ld = 5 * nw + 3
    at = rec_new0.size
    if inp["s1h"]:
        B["s1h"], t.s1h_out = pitched(R_, nsp, nsp + 4, out=True, start=at); t.s1h_ld = nsp + 4; at += B["s1h"].before.size
    if inp["rnn"]:
        B["hid"], t.hid = pitched(R_, nh, nh + 8, inp["hid"]); t.hid_ld = nh + 8
        B["add"], t.add = pitched(R_, nh, nh + 3, inp["add"]); t.add_ld = nh + 3
        B["out"], t.out = pitched(R_, nh, nh + 12, out=True, start=at); t.out_ld = nh + 12
    hd.check(hd.lib.sqair_slot_tail_test(hd.h, C.byref(t), stream()), "sqair_slot_tail_test")
    for name, b in B.items():
        b.check_untouched(name)
    rn = B["rec_new"].after()
    got = dict(logit=rn[:, slot, L["LOGIT"]][:, None], prob=rn[:, slot, L["PROB"]][:, None], pres=rn[:, slot, L["PRES"]])
    for k, col in (("what", "WHAT"), ("what_loc", "WHAT_LOC"), ("what_scale", "WHAT_SCALE")):
        got[k] = rn[:, slot, L[col]:L[col] + nw]
    if inp["s1h"]:
        got["s1h"] = B["s1h"].p.view(B["s1h"].after())
    if inp["rnn"]:
        got["out"] = B["out"].p.view(B["out"].after())
    got["rec_new"] = rn
    return got


TAIL_CASES = {   # name: (handle, is_disc, slot, R, what_done, s1h_out, seed)
    "disc s0 R1 nw50 s1h": ("f_50_256", 1, 0, 1, 0, 1, 1),
    "disc s2 R17 nw50 wd": ("f_50_256", 1, 2, 17, 1, 0, 2),
    "prop s0 R37 nw50": ("f_50_256", 0, 0, 37, 0, 0, 3),
    "prop s3 R16 nw50 wd s1h": ("f_50_256", 0, 3, 16, 1, 1, 4),
    "disc s1 R5 nw7 nh128 s1h": ("f_7_128", 1, 1, 5, 0, 1, 5),
    "prop s2 R37 nw7 nh128 wd": ("f_7_128", 0, 2, 37, 1, 0, 6),
    "disc s0 R16 nw1": ("f_1_256", 1, 0, 16, 0, 0, 7),
    "prop s1 R17 nw1 s1h": ("f_1_256", 0, 1, 17, 0, 1, 8),
    "disc s2 R37 nw10 nh128": ("f_10_128", 1, 2, 37, 0, 0, 9),
    "prop s0 R5 nw10 nh128 wd s1h": ("f_10_128", 0, 0, 5, 1, 1, 10),
    "disc s1 R17 nw33 wd s1h": ("f_33_256", 1, 1, 17, 1, 1, 11),
    "prop s2 R1 nw33": ("f_33_256", 0, 2, 1, 0, 0, 12),
    "wide disc s1 R17 nw64": ("f_64_256_wide", 1, 1, 17, 0, 0, 13),
    "wide prop s13 R5 nw65 nh512 s1h": ("f_65_512_wide", 0, 13, 5, 0, 1, 14),
    "wide disc s0 R16 nw65 nh512": ("f_65_512_wide", 1, 0, 16, 0, 0, 15),
    "wide prop s2 R37 nw128 s1h": ("f_128_256_wide", 0, 2, 37, 0, 1, 16),
}
RNN_CASES = {k: v for k, v in TAIL_CASES.items() if not k.startswith("wide") and v[2] + 1 < HANDLES[v[0]][2]}
RNN_CASES = {k: v + (True, None) for k, v in RNN_CASES.items()}
RNN_CASES.update({   # below and at the switch to two column tiles per workgroup (257 tiles): the R256 / R512 cases are the first rows
    "disc s1 R259 nw50": ("f_50_256", 1, 1, 259, 0, 0, 21, True, None),          # of the R259 / R515 ones
    "disc s1 R256 nw50": ("f_50_256", 1, 1, 259, 0, 0, 21, True, 256),
    "prop s0 R515 nw7 nh128 wd": ("f_7_128", 0, 0, 515, 1, 0, 22, True, None),
    "prop s0 R512 nw7 nh128 wd": ("f_7_128", 0, 0, 515, 1, 0, 22, True, 512),
})


@pytest.mark.parametrize("case", sorted(TAIL_CASES))
def test_slot_tail(case):
    c = cases("slot_tail")[case]
    _judge("slot_tail", case, run_tail(c), c)


@pytest.mark.parametrize("case", sorted(RNN_CASES))
def test_rnn_tail(case):
    c = cases("rnn_tail")[case]
    _judge("rnn_tail", case, run_tail(c), c)


def _plain_layer(hd, x, w, b, M, N_, act_b=0, act_split=1 << 30, add=None):
    """out [M, N_] = act(x w + b (+ add)) through sqair_linear_contract_test: the dense launcher on the same operands."""
    kc, nt = sum((k + 15) // 16 for k in [s.shape[1] for s in x]), (N_ + 15) // 16
    scratch = torch.zeros(2 * nt * kc * 256 + 32 * nt + 256 + 64, device="cuda")
    out = torch.full((M, N_), float("nan"), device="cuda")
    c = _capi.SqairDenseContract()
    c.nseg = len(x)
    for i, s in enumerate(x):
        assert s.is_contiguous() and s.shape[1] % 4 == 0
        c.seg[i].p, c.seg[i].ld, c.seg[i].width, c.seg[i].rdiv = s.data_ptr(), s.shape[1], s.shape[1], 1
    wd_, bd = torch.from_numpy(np.ascontiguousarray(w, F32)).cuda(), torch.from_numpy(np.ascontiguousarray(b, F32)).cuda()
    c.w, c.b = wd_.data_ptr(), bd.data_ptr()
    if add is not None:
        c.add, c.add_ld, c.add_n, c.add_rdiv = add.data_ptr(), add.shape[1], N_, 1
    c.act_a, c.act_b, c.act_split, c.scale = (2 if add is not None else 0), act_b, act_split, 1.0
    c.out, c.out_ld, c.M, c.N = out.data_ptr(), N_, M, N_
    c.scratch, c.scratch_bytes = scratch.data_ptr(), scratch.numel() * 4
    hd.check(hd.lib.sqair_linear_contract_test(hd.h, C.byref(c), stream()), "sqair_linear_contract_test")
    return out


@pytest.mark.parametrize("case", sorted(RNN_CASES))
def test_rnn_tail_is_the_tail_and_then_the_plain_layer(case):
    """The claim of the comment above k_rnn_tail: `out` and the record bit for bit equal k_slot_tail followed by the layer through the
    dense launcher on the same pack contents and operands."""
    c = cases("rnn_tail")[case]
    inp = c["inp"]
    hd = handle(inp["hname"])
    L, nw, nh, slot, R_ = hd.L, hd.nw, hd.nh, inp["slot"], inp["R"]
    core = "disc" if inp["is_disc"] else "prop"
    fused = run_tail(c)
    alone = run_tail(dict(c, inp=dict(inp, rnn=False)))
    assert np.array_equal(_bits(fused["rec_new"]), _bits(alone["rec_new"])), "the records differ"
    if inp["s1h"]:
        assert np.array_equal(_bits(fused["s1h"]), _bits(alone["s1h"]))
    # the layer's matrix in the kernels' row order: the z-record (56 rows: where | what, padded to 50 | presence | logit), then h2h
    ZW = L["LOGIT"] + 1 - L["WHERE"]
    wz = np.zeros((ZW, nh), F32)
    Wi = inp["P"][core + ".rnn.i2h.w"]
    for f, col, n in (("where", L["WHERE"], 4), ("what", L["WHAT"], nw), ("pres", L["PRES"], 1)):
        r0, r1 = SF.rows_of(SF.RNN_INPUT[core], f, nh, nw)
        wz[col - L["WHERE"]:col - L["WHERE"] + n] = Wi[r0:r1]
    z = np.zeros((R_, ZW), F32)
    z[:] = alone["rec_new"][:, slot, L["WHERE"]:L["WHERE"] + ZW]
    z[:, L["WHAT"] - L["WHERE"] + nw:L["PRES"] - L["WHERE"]] = 0.0                 # (what columns beyond n_what: zero in the kernel's tile)
    out = _plain_layer(hd, [dev(z), dev(inp["hid"])], np.concatenate([wz, inp["P"][core + ".rnn.h2h.w"]], 0), np.zeros(nh, F32), R_, nh,
                       add=dev(inp["add"]))
    assert np.array_equal(_bits(fused["out"]), _bits(out.cpu().numpy())), "the layer's output differs"


@pytest.mark.parametrize("big,small", [("disc s1 R259 nw50", "disc s1 R256 nw50"), ("prop s0 R515 nw7 nh128 wd", "prop s0 R512 nw7 nh128 wd")])
def test_rnn_tail_two_column_tiles_equal_one(big, small):
    """The launch with two column tiles per workgroup (from 257 tiles on) equals, on its first rows, those rows launched with one."""
    cs = cases("rnn_tail")
    two, one = run_tail(cs[big]), run_tail(cs[small])
    n = cs[small]["inp"]["R"]
    assert n < cs[big]["inp"]["R"]
    for k in ("out", "logit", "prob", "pres", "what", "what_loc", "what_scale"):
        assert np.array_equal(_bits(two[k][:n]), _bits(one[k])), k


# ------------------------------------------------------------------------------------------------ k_linear_what
WHAT_CASES = {}   # name: (handle, mode, slot, B, seed)
for _i, (_h, _m, _s, _B) in enumerate([("f_50_256", 0, 0, 17), ("f_50_256", 1, 3, 160), ("f_50_256", 1, 1, 1), ("f_1_256", 0, 2, 160),
                                       ("f_1_256", 1, 0, 17), ("f_3_128", 0, 1, 1), ("f_3_128", 1, 2, 160), ("f_10_128", 0, 0, 160),
                                       ("f_10_128", 1, 1, 17), ("f_33_256", 0, 2, 1), ("f_33_256", 1, 0, 160), ("f_7_128", 1, 2, 17),
                                       ("f_50_128_k17", 0, 1, 353), ("f_50_128_k17", 1, 0, 353)]):
    WHAT_CASES["mode%d %s s%d M%d" % (_m, _h[2:], _s, _B * HANDLES[_h][3])] = (_h, _m, _s, _B, 40 + _i)


def build_what(hname, mode, slot, B_, seed):
    hd = handle(hname)
    nw, nh, N, M = hd.nw, hd.nh, hd.N, B_ * hd.K
    rng = np.random.default_rng(7000 + seed)
    x = _f32(np.tanh(rng.standard_normal((M, nh))))
    col = lambda n, s: rng.standard_normal((nh, n)) * s / np.sqrt(nh)
    if mode == 0:   # pre-activations: loc ~ N(0, 1), raw scale over [-12, 10]
        P = {"enc.what_head.w": _f32(np.concatenate([col(nw, 1.5), col(nw, 3.0)], 1)),
             "enc.what_head.b": _f32(np.concatenate([rng.standard_normal(nw) * 0.3, rng.uniform(-10, 8, size=nw)]))}
    else:           # gates out to +-20
        P = {"prop.what_head.w": _f32(np.concatenate([col(nw, 1.5), col(nw, 3.0)], 1)),
             "prop.what_head.b": _f32(np.concatenate([rng.standard_normal(nw) * 0.3, rng.uniform(-10, 8, size=nw)])),
             "prop.gates.w": _f32(col(3 * nw, 4.0)), "prop.gates.b": _f32(rng.uniform(-16, 16, size=3 * nw))}
        # element 0 of each gate is surely not saturated: a row of saturated gates only has no scale to measure against but the
        # rounding of 1 - sigmoid (in any fp32 evaluation)
        P["prop.gates.w"][:, ::nw] *= F32(0.1)
        P["prop.gates.b"][::nw] = _f32(rng.uniform(-1, 1, size=3))
    L, W = hd.L, hd.L["W"]
    rec_prev = np.full((M, N, W), np.nan, F32)
    enc = None
    if mode == 1:
        rec_prev[:, slot, L["WHAT"]:L["WHAT"] + nw] = _f32(rng.standard_normal((M, nw)))
        enc = _f32(np.concatenate([rng.standard_normal((M, nw)), _scales(rng, (M, nw))], -1))
    noise = np.full((M, 2, N, hd.nzw), np.nan, F32)
    noise[:, 1 - mode, slot, 4:4 + nw] = _f32(rng.standard_normal((M, nw)))
    inp = dict(hname=hname, mode=mode, slot=slot, B=B_, R=M, P=P, x=x, enc=enc, rec_prev=rec_prev, rec_new=_sentinel_records(M, N, W, 0), noise=noise)
    return _finish("linear_what", inp)


def eval_what(inp, dtype):
    hd = handle(inp["hname"])
    nw, is_disc = hd.nw, inp["mode"] == 0
    P = SF.params(inp["P"], dtype)
    ops = SF.slot_operands(inp["rec_prev"], inp["rec_new"], inp["noise"], hd.L, is_disc, inp["slot"], nw, dtype)
    if is_disc:
        ops["prev"] = torch.ones(inp["R"], dtype=dtype)              # (the previous presence is not an operand of the sample)
    x = R.T(inp["x"], dtype)
    # what and what_loc are sums that cancel (a K = n_hidden product, the gated mixture), and with n_what = 1 a row has no neighbour to
    # take a scale from: they are judged on their absolute terms.  what_scale is a sum of positive terms.
    if is_disc:
        loc, scale = SF.gaussian_head(P, "enc.what_head", x)
        out = SF.what_sample(ops, True, loc, scale)
        terms = x.abs() @ P["enc.what_head.w"][:, :nw].abs() + P["enc.what_head.b"][:nw].abs()
    else:
        enc = R.T(inp["enc"], dtype)
        hraw = SF.prop_heads_raw(P, x)
        out = SF.what_sample(ops, False, enc[:, :nw], enc[:, nw:], hraw)
        g = R.gates_of(hraw[:, 2 * nw:])
        t_loc = x.abs() @ P["prop.what_head.w"][:, :nw].abs() + P["prop.what_head.b"][:nw].abs()
        terms = g[:, :nw].abs() * ops["what_tm1"].abs() + (1.0 - g[:, nw:2 * nw]).abs() * enc[:, :nw].abs() + (1.0 - g[:, 2 * nw:]).abs() * t_loc
    out["what_loc_terms"] = terms
    out["what_terms"] = terms + out["what_scale"] * ops["eps"].abs()
    return SF.np64(out)


def run_what(c):
    inp = c["inp"]
    hd = handle(inp["hname"])
    L, nw, nh, M, slot, mode = hd.L, hd.nw, hd.nh, inp["R"], inp["slot"], inp["mode"]
    flat = Buf(hd.flat_of(inp["P"]))
    packed = hd.pack(flat)
    own = np.zeros(inp["rec_new"].shape, bool)
    for k in ("WHAT", "WHAT_LOC", "WHAT_SCALE"):
        own[:, slot, L[k]:L[k] + nw] = True
    B = dict(flat=flat, rec_new=Buf(inp["rec_new"], own), rec_prev=Buf(inp["rec_prev"]), noise=Buf(inp["noise"]))
    t = _capi.SqairLinearWhatTest()
    t.mode, t.slot, t.B = mode, slot, inp["B"]
    t.rec_new, t.noise, t.packed = B["rec_new"].ptr(), B["noise"].ptr(), packed
    B["x"], t.x = pitched(M, nh, nh + 8, inp["x"]); t.x_ld = nh + 8
    if mode == 1:
        t.rec_prev = B["rec_prev"].ptr()
        B["enc"], t.enc = pitched(M, 2 * nw, 2 * nw + 5, inp["enc"]); t.enc_ld = 2 * nw + 5
    hd.check(hd.lib.sqair_linear_what_test(hd.h, C.byref(t), stream()), "sqair_linear_what_test")
    for name, b in B.items():
        b.check_untouched(name)
    rn = B["rec_new"].after()
    got = {k: rn[:, slot, L[col]:L[col] + nw] for k, col in (("what", "WHAT"), ("what_loc", "WHAT_LOC"), ("what_scale", "WHAT_SCALE"))}
    got["rec_new"] = rn
    return got


@pytest.mark.parametrize("case", sorted(WHAT_CASES))
def test_linear_what(case):
    c = cases("linear_what")[case]
    _judge("linear_what", case, run_what(c), c)


@pytest.mark.parametrize("case", sorted(k for k, v in WHAT_CASES.items() if v[3] * HANDLES[v[0]][3] < 6000))
def test_linear_what_then_the_tail_is_the_plain_head_then_the_tail(case):
    """Below the row count at which the plain head layers leave the split-K kernel: the tail with what_done on k_linear_what's output
    equals, bit for bit, the tail deriving the sample from the plain head layer's output (the claim above WhatArgs, sqair_glue.h)."""
    c = cases("linear_what")[case]
    inp = c["inp"]
    hd = handle(inp["hname"])
    nw, nh, M, slot, mode = hd.nw, hd.nh, inp["R"], inp["slot"], inp["mode"]
    fused = run_what(c)
    # the tail's other operands: any finite values, the same for both
    rng = np.random.default_rng(99)
    core = "disc" if mode == 0 else "prop"
    P = dict(inp["P"], **_steps_params(rng, core, nh, nw, hd.shapes))
    prev = _prev(rng, M, mode == 0, slot)
    rec_prev, rec_new = inp["rec_prev"].copy(), inp["rec_new"].copy()
    if mode == 0 and slot > 0:
        rec_new[:, slot - 1, hd.L["PRES"]] = prev
    if mode == 1:
        rec_prev[:, slot, hd.L["PRES"]] = prev
    noise = inp["noise"].copy()
    noise[:, 1 - mode, slot, 4 + nw] = _f32(rng.uniform(size=M))
    x = dev(inp["x"])
    if mode == 0:    # L_WHAT_HEAD: loc | softplus(raw) + 1e-2 (activation code 4 from column n_what on)
        enc = _plain_layer(hd, [x], P["enc.what_head.w"], P["enc.what_head.b"], M, 2 * nw, act_b=4, act_split=nw).cpu().numpy()
        hraw = None
    else:            # L_PROP_HEADS: the five raw blocks
        enc = inp["enc"]
        hraw = _plain_layer(hd, [x], np.concatenate([P["prop.what_head.w"], P["prop.gates.w"]], 1),
                            np.concatenate([P["prop.what_head.b"], P["prop.gates.b"]]), M, 5 * nw).cpu().numpy()
    base = dict(hname=inp["hname"], is_disc=mode == 0, slot=slot, R=M, s1h=True, rnn=False, P=P, rec_prev=rec_prev, noise=noise,
                s1p=_f32(rng.standard_normal((M, nh // 2))), hid=None, add=None)
    start = rec_new.copy()
    for k in ("WHAT", "WHAT_LOC", "WHAT_SCALE"):
        start[:, slot, hd.L[k]:hd.L[k] + nw] = fused["rec_new"][:, slot, hd.L[k]:hd.L[k] + nw]
    a = run_tail(dict(inp=dict(base, wd=True, enc=enc, hraw=hraw if hraw is not None else None, rec_new=rec_new)), what_done_from=start)
    b = run_tail(dict(inp=dict(base, wd=False, enc=enc, hraw=hraw, rec_new=rec_new)))
    assert np.array_equal(_bits(a["rec_new"]), _bits(b["rec_new"])), "the records differ"
    assert np.array_equal(_bits(a["s1h"]), _bits(b["s1h"]))


# ------------------------------------------------------------------------------------------------ crop
SPECIAL_WHERE = np.array([[2.0, 1.5, 12.0, -12.0], [3.0, 3.0, -2.5, 2.5], [-12.0, -10.0, 0.3, -0.2], [-1.0, 2.0, 4.0, 0.3]], F32)
CROP_CASES = {}   # name: (handle, B, mode, slot, mask, fused, tp_out, specialised, seed)
for _i, (_h, _B) in enumerate([("k_50x50", 8), ("k_37x41_g12", 8), ("k_64x64_g28", 7), ("k_72x64_128", 8), ("k_3x250", 7), ("k_257x5_g12", 7),
                               ("k_50x50_512_wide", 3)]):
    _N = HANDLES[_h][2]
    _s = 20 * _i
    CROP_CASES[_h + " prop1 mask"] = (_h, _B, 1, 0, 1, 0, 0, 0, _s + 1)
    CROP_CASES[_h + " prop2 s%d mask fused tp_out" % (_N - 1)] = (_h, _B, 2, _N - 1, 1, 1, 1, 0, _s + 2)
    CROP_CASES[_h + " disc s0 tp"] = (_h, _B, 3, 0, 0, 0, 0, 0, _s + 3)
CROP_CASES.update({
    "k_50x50 prop1 no mask": ("k_50x50", 8, 1, 0, 0, 0, 0, 0, 4),
    "k_50x50 prop2 s0 no mask tp": ("k_50x50", 8, 2, 0, 0, 0, 0, 0, 5),
    "k_50x50 disc s2 mask fused": ("k_50x50", 8, 3, 2, 1, 1, 0, 0, 6),
    "k_50x50 disc s1 fused tp_out": ("k_50x50", 8, 3, 1, 0, 1, 1, 0, 7),
    "k_50x50 prop2 s1 mask fused": ("k_50x50", 8, 2, 1, 1, 1, 0, 0, 8),
    "k_37x41_g12 disc s1 fused B7": ("k_37x41_g12", 7, 3, 1, 0, 1, 1, 0, 9),
    "k_64x64_g28 prop2 s0 mask tp B8": ("k_64x64_g28", 8, 2, 0, 1, 0, 0, 0, 10),
})
SPEC_PAIRS = ("k_50x50 prop1 mask", "k_50x50 prop2 s1 mask fused", "k_50x50 disc s1 fused tp_out")
for _k in SPEC_PAIRS:
    CROP_CASES[_k + " specialised"] = CROP_CASES[_k][:7] + (1,) + CROP_CASES[_k][8:]


def _where_targets(rng, rows):
    """Where logits to aim at: saturated shifts with large scales (mostly outside the frame), the 1e-4 floor of the scale, ordinary."""
    w = rng.standard_normal((rows, 4)) * np.array([1.0, 1.0, 0.8, 0.8]) + np.array([-0.5, -0.5, 0.0, 0.0])
    k = min(rows, len(SPECIAL_WHERE))
    w[:k] = SPECIAL_WHERE[:k]
    return w


def build_crop(hname, B_, mode, slot, mask, fused, tp_out, spec, seed):
    hd = handle(hname)
    (H, W), N, K, G, nh = hd.hw, hd.N, hd.K, hd.G, hd.nh
    R_ = B_ * K
    rng = np.random.default_rng(9000 + seed)
    L, RW = hd.L, hd.L["W"]
    core = "disc" if mode == 3 else "prop"
    img = _image(rng, B_, H, W)
    nsl = N if mode == 1 else 1
    rec_prev = np.full((R_, N, RW), np.nan, F32)
    rec_new = _sentinel_records(R_, N, RW, 0)
    noise = np.full((R_, 2, N, hd.nzw), np.nan, F32)
    P, tp, t2, wb = {}, None, None, None
    W0 = L["WHERE"]
    if mode == 1:
        wb = _f32(rng.standard_normal((R_ * N, 4)) * 3.0)
        rec_prev[:, :, W0:W0 + 4] = _f32(_where_targets(rng, R_ * N) - 0.1 * wb).reshape(R_, N, 4)
    else:
        noise[:, mode - 2, slot, :4] = _f32(rng.standard_normal((R_, 4)))
        # the transform's output: loc at the where targets, raw scales from -12 to 6
        tp = np.concatenate([_where_targets(rng, R_), rng.uniform(-12.0, 6.0, size=(R_, 4))], 1)
        if mode == 2:
            where_tm1 = _f32(rng.standard_normal((R_, 4)) * 0.5)
            rec_prev[:, slot, W0:W0 + 4] = where_tm1
            tp[:, :4] -= where_tm1
            P["prop.cholesky_scale"] = CHOLESKY
        P[core + ".transform.scale_offset"] = np.asarray(SCALE_OFFSET[mode], F32).reshape(hd.shapes[core + ".transform.scale_offset"])
        tp = _f32(tp)
        if fused:    # t2 and an output layer that land on tp: w3 random, the bias takes the rows' mean, the rest goes into 8 of t2's units
            t2 = _f32(O.elu(torch.as_tensor(rng.standard_normal((R_, nh)))).numpy())
            w3 = rng.standard_normal((nh, 8)) * 0.5 / np.sqrt(nh)
            w3[:8] = np.eye(8)
            t2[:, :8] = 0.0
            t2[:, :8] = _f32(tp - t2.astype(F64) @ w3)
            P[core + ".transform.l2.w"], P[core + ".transform.l2.b"] = _f32(w3), np.zeros(8, F32)
            tp = None
    mk = _f32(rng.uniform(0.05, 0.95, size=(R_ * nsl, G * G))) if mask else None
    inp = dict(hname=hname, B=B_, R=R_, mode=mode, slot=slot, spec=spec, fused=bool(fused), tp_out=bool(tp_out), P=P, img=img, tp=tp, t2=t2,
               wb=wb, mask=mk, rec_prev=rec_prev, rec_new=rec_new, noise=noise)
    return _finish("crop", inp)


def eval_crop(inp, dtype):
    hd = handle(inp["hname"])
    (H, W), N, K, G, mode, slot, R_ = hd.hw, hd.N, hd.K, hd.G, inp["mode"], inp["slot"], inp["R"]
    P = SF.params(inp["P"], dtype)
    img = R.T(inp["img"], dtype)
    W0 = hd.L["WHERE"]
    rp = R.T(inp["rec_prev"], dtype)
    if mode == 1:   # row (r, k) of the launch: frame r // K
        rows = img[torch.arange(R_ * N) // (N * K)]
        lv = dict(where_tm1=rp[:, :, W0:W0 + 4].reshape(R_ * N, 4), wb=R.T(inp["wb"], dtype))
        c = dict(img=rows, G=G, mode=1)
    else:
        ops = SF.slot_operands(inp["rec_prev"], inp["rec_new"], inp["noise"], hd.L, mode == 3, slot, hd.nw, dtype)
        core = "disc" if mode == 3 else "prop"
        tp = SF.transform_out(P, core, R.T(inp["t2"], dtype)) if inp["fused"] else R.T(inp["tp"], dtype)
        lv = dict(tp=tp, bump=torch.zeros(R_, 4, dtype=dtype))
        c = dict(img=img[torch.arange(R_) // K], G=G, mode=mode, scale_offset=P[core + ".transform.scale_offset"].reshape(()), eps=ops["eps_where"])
        if mode == 2:
            lv["where_tm1"] = ops["where_tm1"]
            c["cholesky"] = P["prop.cholesky_scale"]
    if inp["mask"] is not None:
        lv["mask"] = R.T(inp["mask"], dtype)
    o = R.crop_forward(lv, c)
    out = dict(glimpse=o["glimpse"])
    if mode != 1:
        out.update(where=o["where"], where_loc=o["where_loc"], where_scale=o["where_scale"])
        if inp["fused"] and inp["tp_out"]:
            out["tp_out"] = o["tp"]
    return SF.np64(out)


def run_crop(c):
    inp = c["inp"]
    hd = handle(inp["hname"])
    (H, W), N, K, G, nh, mode, slot, R_, B_ = hd.hw, hd.N, hd.K, hd.G, hd.nh, inp["mode"], inp["slot"], inp["R"], inp["B"]
    L, G2 = hd.L, hd.G * hd.G
    nsl = N if mode == 1 else 1
    flat = Buf(hd.flat_of({k: v for k, v in inp["P"].items() if "transform.l2" not in k}))
    P4 = (H * W + 3) // 4 * 4
    frames, fptr = pitched(B_, H * W, P4, inp["img"].reshape(B_, H * W))    # (the padding of a frame is never read: NaN)
    own = np.zeros(inp["rec_new"].shape, bool)
    if mode != 1:
        for k in ("WHERE", "WHERE_LOC", "WHERE_SCALE"):
            own[:, slot, L[k]:L[k] + 4] = True
    B = dict(flat=flat, frames=frames, rec_new=Buf(inp["rec_new"], own), rec_prev=Buf(inp["rec_prev"]), noise=Buf(inp["noise"]))
    t = _capi.SqairSlotCropTest()
    t.mode, t.slot, t.B, t.specialised = mode, slot, B_, inp["spec"]
    t.img, t.flat, t.rec_prev = fptr, flat.ptr(), B["rec_prev"].ptr()
    # the glimpses of a launch: row r (slot k) at row r * mul + add (+ k) of a taller buffer; the rows between are not written
    mul, add = nsl + 1, 1
    B["out"] = Buf(R.distinct_words((R_ * mul + add + 2) * G2, inp["rec_new"].size).reshape(-1, G2).copy())
    orow = (np.arange(R_)[:, None] * mul + add + np.arange(nsl)[None, :]).reshape(-1)
    B["out"].owned[orow] = True
    t.out, t.out_row_mul, t.out_row_add = B["out"].ptr(), mul, add
    if inp["mask"] is not None:
        mm, ma = nsl + 2, 2
        host = np.full((R_ * mm + ma + 2, G2), np.nan, F32)
        host[(np.arange(R_)[:, None] * mm + ma + np.arange(nsl)[None, :]).reshape(-1)] = inp["mask"]
        B["mask"] = Buf(host)
        t.mask, t.mask_row_mul, t.mask_row_add = B["mask"].ptr(), mm, ma
    if mode == 1:
        B["wb"], t.wb = pitched(R_ * N, 4, 7, inp["wb"]); t.wb_ld = 7
    else:
        t.rec_new, t.noise = B["rec_new"].ptr(), B["noise"].ptr()
        if inp["fused"]:
            core = "disc" if mode == 3 else "prop"
            B["t2"], t.t2 = pitched(R_, nh, nh + 8, inp["t2"]); t.t2_ld = nh + 8
            B["w3"] = Buf(np.concatenate([inp["P"][core + ".transform.l2.w"].reshape(-1), inp["P"][core + ".transform.l2.b"], np.full(8, np.nan, F32)]))
            t.w3 = B["w3"].ptr()
            if inp["tp_out"]:
                B["tp_out"], t.tp_out = pitched(R_, 8, 11, out=True, start=inp["rec_new"].size + B["out"].before.size); t.tp_out_ld = 11
        else:
            B["tp"], t.tp = pitched(R_, 8, 9, inp["tp"]); t.tp_ld = 9
    hd.check(hd.lib.sqair_slot_crop_test(hd.h, C.byref(t), stream()), "sqair_slot_crop_test")
    for name, b in B.items():
        b.check_untouched(name)
    got = dict(glimpse=B["out"].after()[orow])
    if mode != 1:
        rn = B["rec_new"].after()
        got.update(where=rn[:, slot, L["WHERE"]:L["WHERE"] + 4], where_loc=rn[:, slot, L["WHERE_LOC"]:L["WHERE_LOC"] + 4],
                   where_scale=rn[:, slot, L["WHERE_SCALE"]:L["WHERE_SCALE"] + 4])
        if inp["fused"] and inp["tp_out"]:
            got["tp_out"] = B["tp_out"].p.view(B["tp_out"].after())
    return got


@pytest.mark.parametrize("case", sorted(CROP_CASES))
def test_crop(case):
    c = cases("crop")[case]
    _judge("crop", case, run_crop(c), c)


@pytest.mark.parametrize("case", SPEC_PAIRS)
def test_crop_specialised_equals_generic(case):
    """The instantiation with the shipped family's dimensions compiled in against the generic one: every output bit for bit (and the
    specialised launch was one: the library counts them)."""
    cs = cases("crop")
    hd = handle(cs[case]["inp"]["hname"])
    count = lambda: int(hd.lib.sqair_debug_specialised_launches())
    n0 = count()
    gen = run_crop(cs[case])
    n1 = count()
    spec = run_crop(cs[case + " specialised"])
    assert n1 == n0 and count() == n1 + 1
    assert set(gen) == set(spec)
    for k in gen:
        assert np.array_equal(_bits(gen[k]), _bits(spec[k])), k


CASES = dict(slot_tail=TAIL_CASES, rnn_tail=RNN_CASES, linear_what=WHAT_CASES, crop=CROP_CASES)
BUILD = dict(slot_tail=build_tail, rnn_tail=build_tail, linear_what=build_what, crop=build_crop)
EVAL = dict(slot_tail=eval_tail, rnn_tail=eval_tail, linear_what=eval_what, crop=eval_crop)
