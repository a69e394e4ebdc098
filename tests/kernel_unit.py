"""The harness of the kernel unit tests (tests/test_slot_adjoint_kernels.py, test_slot_forward_kernels.py, test_logprob_kernels.py, and
the forward layer and parity file of test_dense_contract.py and test_linear_strip.py): handles on the unit entries of
sqair_unit_test.hip, device buffers that know which words the kernel owns, the per-file figures and their JSON, the judge, the case
cache and the bars.  Importable without a GPU: the CPU tests build
the test modules' cases and bars through it; only Buf, Handle.pack and a test's own launches touch the device.

What differs by file stays with the file and comes in as an argument: the error metric and the per-output scales, which outputs are
exact, which of a case's float32 figures a kernel's bar is taken from."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from sqair_amd.params import param_spec
from tests import slot_adjoint_ref as R
from tests.hip_util import dev, stream

PARITY_DIR_ENV = "SQAIR_PARITY_DIR"
LAYOUT = ("W", "PRES", "ID", "WHERE", "WHAT", "LOGIT", "WHERE_LOC", "WHERE_SCALE", "WHAT_LOC", "WHAT_SCALE", "PROB", "snh", "psnh",
          "n_flat", "temporal_init", "prior_init", "max_slots", "N", "nw", "spec_ok")
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------ handles
class Handle:
    """A library handle of one configuration with what the tests read off it: the record layout (L), the parameter offsets (off) and
    the oracle's shapes (shapes), the noise width (nzw)."""

    def __init__(self, name, wide, hw, N, K, flags):
        self.name, self.hw, self.N, self.K, self.wide = name, hw, N, K, wide
        self.lib = _capi.lib(_capi.WIDE_LIB_PATH if wide else _capi.LIB_PATH)
        self.F = make_flags(k_particles=K, n_steps_per_image=N, **flags)
        self.cfg = make_config(self.F, hw)
        self.h = C.c_void_p()
        assert self.lib.sqair_create(C.byref(self.cfg), C.byref(self.h)) == 0, name
        buf = (C.c_int32 * 20)()
        assert self.lib.sqair_compact_test_layout(self.h, buf, 20) == 20
        self.L = dict(zip(LAYOUT, [int(v) for v in buf]))
        self.nw, self.nh, self.G = int(self.cfg.n_what), int(self.cfg.n_hidden), int(self.cfg.glimpse_size)
        self.nzw = self.lib.sqair_noise_width(self.h)
        assert self.L["N"] == N and self.L["nw"] == self.nw and self.nzw == 4 + self.nw + 1
        # n_hidden is not padded in these configurations: the kernels' parameter layout is the caller's
        assert self.L["n_flat"] == self.lib.sqair_param_count(self.h) == self.lib.sqair_debug_padded_count(self.h, None)
        self.off = {}
        for i in range(self.lib.sqair_param_entries(self.h)):
            cname, coff, cnum = C.c_char_p(), C.c_int64(), C.c_int64()
            assert self.lib.sqair_param_entry(self.h, i, C.byref(cname), C.byref(coff), C.byref(cnum)) == 0
            self.off[cname.value.decode()] = (int(coff.value), int(cnum.value))
        self.shapes = {n: tuple(s) for n, s, _, _ in param_spec(self.F, hw)}    # the oracle's shapes
        self.packed = None

    def check(self, rc, what):
        assert rc == 0, (what, rc, self.lib.sqair_last_error(self.h))

    def flat_of(self, P):
        """The flat parameter buffer: NaN but for the parameters of P (which may hold NaN rows themselves)."""
        flat = np.full(self.L["n_flat"], np.nan, F32)
        for name, v in P.items():
            o, n = self.off[name]
            assert tuple(np.shape(v)) == self.shapes[name] and n == int(np.prod(self.shapes[name], dtype=np.int64)), name
            flat[o:o + n] = np.asarray(v, F32).reshape(-1)
        return flat

    def pack(self, flat_buf):
        if self.packed is None:
            self.packed = torch.zeros(self.lib.sqair_packed_bytes(self.h) // 4, dtype=torch.float32, device="cuda")
        self.check(self.lib.sqair_pack_params(self.h, flat_buf.ptr(), self.packed.data_ptr(), stream()), "sqair_pack_params")
        torch.cuda.synchronize()
        return self.packed.data_ptr()


_open = {}


def handle(name, make):
    """The open handle called `name`; make(name) opens it the first time."""
    if name not in _open:
        _open[name] = make(name)
    return _open[name]


def close():
    for hd in _open.values():
        hd.lib.sqair_destroy(hd.h)
    _open.clear()


# ------------------------------------------------------------------------------------------------ buffers
def mixed(rng, shape, lo=-2.0, hi=1.0):
    """Upstream gradients: mixed sign, magnitudes over three decades."""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(lo, hi, size=shape)).astype(F32)


def f32(x):
    return np.asarray(x, F64).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


class Buf:
    """A host array, its device copy, and which of its words the kernel owns.  Words are float32 unless the array holds integers (the
    int32 frame counters)."""

    def __init__(self, host, owned=None):
        self.before = np.ascontiguousarray(host, None if np.asarray(host).dtype.kind in "iu" else F32)
        self.t = torch.from_numpy(self.before.copy()).cuda()
        self.owned = np.zeros(self.before.shape, bool) if owned is None else owned

    def ptr(self, word=0):
        return self.t.data_ptr() + 4 * int(word)

    def after(self):
        return self.t.cpu().numpy()

    def check_untouched(self, name):
        a, b = self.after().view(np.uint32), self.before.view(np.uint32)
        bad = (a != b) & ~self.owned
        assert not bad.any(), "{}: {} words outside the kernel's outputs changed (first at {})".format(name, int(bad.sum()),
                                                                                                        np.argwhere(bad)[0].tolist())


def pitched(rows, width, ld, data=None, out=False, start=0, offset=0, owned_cols=None):
    """(Buf, pointer of element [0, 0]) of a [rows, width] operand at pitch ld with guard rows; inputs padded with NaN, outputs
    with distinct words (owned_cols: the columns of an output the kernel owns, all of them by default)."""
    p = R.Pitched(rows, width, ld, data=data, nan=not out, start=start, offset=offset)
    owned = np.zeros(p.host.shape, bool)
    if out:
        v = owned[1:1 + rows, offset:offset + width]
        v[:, :] = True if owned_cols is None else owned_cols[None, :]
    b = Buf(p.host, owned)
    b.p = p
    return b, b.ptr(p.first_word())


def records(R_, N, W, fill):
    """[R, N, W] records: NaN (fill "nan": inputs) or distinct words from `fill` on (gradient records, records a launch writes into)."""
    if fill == "nan":
        return np.full((R_, N, W), np.nan, F32)
    return R.distinct_words(R_ * N * W, fill).reshape(R_, N, W).copy()


# ------------------------------------------------------------------------------------------------ figures
def merge_parity(file_name, fresh, update):
    """With SQAIR_PARITY_DIR set: update(data) on the JSON there (fresh() where there is none yet), written back."""
    where = os.environ.get(PARITY_DIR_ENV)
    if not where:
        return
    try:
        os.makedirs(where, exist_ok=True)
        path = os.path.join(where, file_name)
        data = json.load(open(path)) if os.path.exists(path) else fresh()
        update(data)
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


class Parity:
    """The figures of one test file: per kernel, case and output the error, the bar and the float32 reference's own error."""

    def __init__(self, file_name, note, worst_ratio=False):
        self.file_name, self.note, self.worst_ratio, self.figures = file_name, note, worst_ratio, {}

    def record(self, kernel, case, output, err, bar, err32):
        self.figures.setdefault(kernel, {}).setdefault(case, {})[output] = dict(err=err, bar=bar, fp32_reference_err=err32,
                                                                                ratio=err / bar if bar > 0 else None)
        print("{} {} {}: err {:.3e} bar {:.3e} (fp32 reference here {:.3e})".format(kernel, case, output, err, bar,
                                                                                  -1.0 if err32 is None else err32))

    def write(self, worst32):
        """worst32(kernel): per output the float32 figure its bar comes from."""
        if not self.figures:
            return

        def fresh():
            data = {"note": self.note, "build_id": _capi.build_id(), "bars": {}, "cases": {}}
            if self.worst_ratio:
                data["worst_ratio"] = {}
            return data

        def update(data):
            for kernel, cases in self.figures.items():
                data["cases"].setdefault(kernel, {}).update(cases)
                data["bars"][kernel] = {k: dict(fp32_reference_worst=v, bar=R.bar_from_fp32(v)) for k, v in worst32(kernel).items()}
                if self.worst_ratio:
                    data["worst_ratio"][kernel] = max(o["ratio"] for c in data["cases"][kernel].values() for o in c.values())

        merge_parity(self.file_name, fresh, update)


def judge(parity, kernel, case, outputs, error, err32, worst, exact=()):
    """Every output under its bar, all of them measured and recorded first.  error(output) is the file's metric with the file's scale
    for that output; the bar of an output is bar_from_fp32(worst[output]), 0 for the outputs in `exact`."""
    errs = {k: error(k) for k in sorted(outputs)}
    over = []
    for k, err in errs.items():
        bar = 0.0 if k in exact else R.bar_from_fp32(worst[k])
        parity.record(kernel, case, k, err, bar, err32[k])
        if not err <= bar:
            over.append((k, err, bar))
    assert not over, "outputs over their bar (name, err, bar): {}".format(over)


# ------------------------------------------------------------------------------------------------ cases, bars
class Cases:
    """The cases of a test file, built once each: build(key) makes the cases {name: case} of one key (a kernel)."""

    def __init__(self, build):
        self.build, self.cache = build, {}

    def __call__(self, key):
        if key not in self.cache:
            self.cache[key] = self.build(key)
        return self.cache[key]


def worst32(cases, field="err32"):
    """Per output: the worst error of the float32 reference (a case's `field`) over the cases."""
    worst = {}
    for c in cases.values():
        for name, e in c[field].items():
            worst[name] = max(worst.get(name, 0.0), e)
    return worst


# ------------------------------------------------------------------------------------------------ the crop cases' shared inputs
CHOLESKY = np.linspace(-0.55, 0.65, 10).astype(F32)
SCALE_OFFSET = {2: F32(-0.7), 3: F32(0.4)}


def image(rng, B_, H, W):
    """Frames in [0, 1] with structure at the scale of a glimpse pixel and above (a few random plane waves) and 10 % white noise."""
    yy, xx = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    img = np.zeros((B_, H, W))
    for b in range(B_):
        for _ in range(6):
            fy, fx, ph = rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(0, 2 * np.pi)
            img[b] += rng.uniform(0.3, 1.0) * np.sin(2 * np.pi * (fy * yy + fx * xx) + ph)
    img = 0.5 + 0.45 * img / np.abs(img).max((1, 2), keepdims=True)
    return f32(np.clip(0.9 * img + 0.1 * rng.uniform(size=img.shape), 0.0, 1.0))


# ------------------------------------------------------------------------------------------------ the dense operand contract
# (tests/test_dense_contract.py and tests/test_linear_strip.py: one forward layer's operands, its launch and what is asserted of it)
NONE, ELU, TANH, SIGMOID, SOFTPLUS_MIN = range(5)


def dense_record(case, **figures):
    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data["cases"][case] = figures

    merge_parity("dense_contract_parity.json", lambda: {
        "note": "per case of tests/test_dense_contract.py: the kernel family the launcher chose, the largest error against the "
                "float64 reference, the bar and err / bar.  Forward errors are absolute; dX errors are relative to the "
                "destination's largest reference value; GRU destinations add `f32_formula_err` (the same formulas in numpy "
                "float32 from the rounded float64 GEMM result) and `allowance` = 4 x that, which is part of their bar.",
        "cases": {}}, update)


@pytest.fixture(scope="module", name="handle")
def dense_handle():
    """The module-scoped handle of the dense contract tests: a test file imports it by name."""
    lib = _capi.lib()
    cfg = make_config(make_flags(k_particles=3, n_steps_per_image=4), (50, 50))
    h = C.c_void_p()
    rc = lib.sqair_create(C.byref(cfg), C.byref(h))
    assert rc == 0, ("sqair_create", rc)
    yield lib, h
    lib.sqair_destroy(h)


def took(before):
    """The routes counted since `before`, as {family: launches}."""
    after = _capi.dense_routes()
    return {k: after[k] - before[k] for k in after if after[k] != before[k]}


def act64(v, act):
    with np.errstate(over="ignore"):
        return [v, np.where(v > 0, v, np.expm1(np.minimum(v, 0))), np.tanh(v), 1.0 / (1.0 + np.exp(-v)),
                np.maximum(v, 0) + np.log1p(np.exp(-np.abs(v))) + 1e-2][act]


RICH = ((20, 5, False), (33, 1, False), (27, 1, True))   # (width, row divisor, broadcast) per segment
SCALE, SCALE_DEV = 0.5, 1.25


class Fwd:
    """One layer's operands on the device (sized for `M` rows; any smaller row count launches on the same buffers) and both
    descriptions of it: rich, and plain (what k_linear_big's vector fast path takes)."""

    def __init__(self, seed, M, segs, N):
        rng = np.random.default_rng(seed)
        self.M, self.segs, self.N = M, segs, N
        self.K = sum(w for w, _, _ in segs)
        self.x, self.ld = [], []
        for width, rdiv, bcast in segs:
            wpad = (width + 3) & ~3
            ld = 0 if bcast else wpad + 4
            buf = rng.standard_normal((1 if bcast else -(-M // rdiv), max(ld, wpad))).astype(np.float32)
            buf[:, width:] *= 1e3   # the pad columns: finite by contract, and nothing may come of them
            self.x.append(buf)
            self.ld.append(ld)
        self.w = (rng.standard_normal((self.K, N)) / np.sqrt(self.K)).astype(np.float32)
        self.b = rng.standard_normal(N).astype(np.float32)
        self.add_ld = ((N + 3) & ~3) + 4
        self.add = rng.standard_normal((M, self.add_ld)).astype(np.float32)
        self.d_x = [dev(x) for x in self.x]
        self.d_w, self.d_b, self.d_add = dev(self.w), dev(self.b), dev(self.add)
        self.d_scale = dev(np.array([SCALE_DEV], np.float32))
        kc, nt = sum((w + 15) // 16 for w, _, _ in segs), (N + 15) // 16
        self.kc, self.nt = kc, nt
        self.scratch = torch.empty(2 * nt * kc * 256 + 32 * nt + 256, dtype=torch.float32, device="cuda")

    def describe(self, rich):
        N = self.N
        if rich:
            return dict(add_n=N - 7, add_rdiv=3, act_a=ELU, act_b=SOFTPLUS_MIN, act_split=N // 2 + 1)
        return dict(add_n=(N - 8) & ~3, add_rdiv=1, act_a=ELU, act_b=NONE, act_split=1 << 30)

    def reference(self, rich, M):
        """(out [M, N], max |pre-activation|) in float64."""
        d = self.describe(rich)
        rows = np.arange(M)
        X = np.concatenate([x[np.zeros(M, int) if bcast else rows // rdiv, :width].astype(F64)
                            for x, (width, rdiv, bcast) in zip(self.x, self.segs)], 1)
        pre = X @ self.w.astype(F64) + self.b.astype(F64)
        pre[:, :d["add_n"]] += self.add[rows // d["add_rdiv"], :d["add_n"]].astype(F64)
        n = np.arange(self.N)
        out = np.where(n < d["act_split"], act64(pre, d["act_a"]), act64(pre, d["act_b"]))
        return out * SCALE * SCALE_DEV, float(np.abs(pre).max())

    def contract(self, rich, M, out, out_ld, seg_ptr=None, seg_ld=None):
        d = self.describe(rich)
        c = _capi.SqairDenseContract()
        c.nseg = len(self.segs)
        for i, (width, rdiv, _) in enumerate(self.segs):
            c.seg[i].p = self.d_x[i].data_ptr() if seg_ptr is None or i else seg_ptr
            c.seg[i].ld = self.ld[i] if seg_ld is None or i else seg_ld
            c.seg[i].width, c.seg[i].rdiv = width, rdiv
        c.w, c.b, c.add = self.d_w.data_ptr(), self.d_b.data_ptr(), self.d_add.data_ptr()
        c.add_ld, c.add_n, c.add_rdiv = self.add_ld, d["add_n"], d["add_rdiv"]
        c.act_a, c.act_b, c.act_split = d["act_a"], d["act_b"], d["act_split"]
        c.scale, c.scale_ptr = SCALE, self.d_scale.data_ptr()
        c.out, c.out_ld, c.M, c.N = out.data_ptr(), out_ld, M, self.N
        c.scratch, c.scratch_bytes = self.scratch.data_ptr(), self.scratch.numel() * 4
        return c

    def bar(self, max_pre):
        return 2e-5 * max(1.0, np.sqrt(self.K / 256.0)) * SCALE * SCALE_DEV * max(1.0, max_pre)


def run_fwd(handle, case, L, rich, M, out_pad, family, ref=None):
    """One launch: route, untouched pad columns, finite and within the bar.  Returns the output's first N columns."""
    lib, h = handle
    out_ld = L.N + out_pad
    out = torch.full((M, out_ld), float("nan"), device="cuda")
    before = _capi.dense_routes()
    rc = lib.sqair_linear_contract_test(h, C.byref(L.contract(rich, M, out, out_ld)), stream())
    assert rc == 0, lib.sqair_last_error(h)
    routes = took(before)
    assert routes == {family: 1}, "{}: meant for {}, the launcher took {}".format(case, family, routes)
    got = out.cpu().numpy()
    assert np.array_equal(bits(got[:, L.N:]), bits(np.full((M, out_pad), np.nan))), case + ": columns beyond N were written"
    ref, max_pre = L.reference(rich, M) if ref is None else ref
    assert np.isfinite(got[:, :L.N]).all(), (case, np.argwhere(~np.isfinite(got[:, :L.N]))[:4].tolist())
    err, bar = float(np.abs(got[:, :L.N].astype(F64) - ref).max()), L.bar(max_pre)
    print("{}: {} max err {:.3e} bar {:.3e} (max |pre| {:.2f})".format(case, family, err, bar, max_pre))
    dense_record(case, family=family, err=err, bar=bar, ratio=err / bar)
    assert err < bar, (case, err, bar)
    return got[:, :L.N]


def segments(kc, nseg):
    """`nseg` segments of `kc` K chunks in all, none a multiple of 16 (nor, but one, of 4) wide; kc = 7 in three segments is the
    rich description itself."""
    if (kc, nseg) == (7, 3):
        return RICH
    chunks = [kc // nseg + (1 if i < kc % nseg else 0) for i in range(nseg)]
    kinds = ((5, False), (1, True)) if nseg == 2 else ((5, False), (1, False), (1, True), (2, False))
    return tuple((16 * c - trim, rdiv, bcast) for c, trim, (rdiv, bcast) in zip(chunks, (12, 15, 5, 3), kinds))
