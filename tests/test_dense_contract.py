"""-m gpu: the dense family against float64, one launch at a time, with the route each launch took asserted.

Forward (sqair_linear_contract_test -> sq_launch_linear): ONE rich operand description -- three segments with pitches wider than
their widths, a row divisor of 5, a plain segment and a broadcast row, an addend on the first N - 7 columns with its own pitch and a
row divisor of 3, ELU below column N // 2 + 1 and softplus + 0.01 above, a host scale and a device scalar, a padded output pitch
(N + 4: 16-byte rows; N + 1: not) -- on every kernel that restates the contract: split-K at every depth it is instantiated for and
every segment count, the 32 x 32 tile, the row-slab, macro-tile and LDS-tiled throughput kernels and the four tile shapes of
k_linear_big, at the smallest shapes the dispatch sends there.  A plain description (4-aligned addend without a divisor, N % 4 == 0,
one activation) reaches k_linear_big's vector fast path.  The output buffer is pre-filled with NaN: columns [N, out_ld) come back
bit for bit, columns [0, N) finite and within the bar.
Bar: test_linear_mfma_matches_fp64's, 2e-5 * max(1, sqrt(K / 256)) absolute on O(1) outputs, inputs drawn as there; times the two
scale factors; times max(1, max |pre-activation|) of the float64 reference, since the addend takes the pre-activations past O(1).

dX (sqair_linear_dx_test -> sq_launch_linear_dx): v = dpre W^T * scale; per range the addend, then the activation derivative from
the saved OUTPUT as dx_dact states it (saved outputs include ELU 0 and -1 + 1e-7, tanh +-1, sigmoid 0 and 1, softplus + 0.01 at its
floor); the GRU gate adjoints of sqair_dx.h.  Every destination starts as NaN (or as known values where the launch accumulates) and
is compared bit for bit outside the rows and columns the launch owns -- the gap between a range's n1 and the next range's n0
included.  Bar: rel_err < 2e-5 per destination (test_linear_backward_mfma's), times sqrt(width / 256) above 256 inputs.  The GRU
epilogue's outputs are products of three or four O(1) factors with no project figure: the same formulas are evaluated in numpy
float32 from the float64 GEMM result rounded to float32, and four times that evaluation's error against float64 is allowed on top.

No element is excluded from a comparison.  With SQAIR_PARITY_DIR set every case appends its family, largest error, bar and their
ratio to dense_contract_parity.json there (the copy under profiles/ is such a file); without it nothing is written."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests.hip_util import dev as _dev, stream
from tests.kernel_unit import (ELU, F64, NONE, RICH, SIGMOID, SOFTPLUS_MIN, TANH, Fwd, act64, bits as _bits,
                               dense_handle as handle, dense_record, run_fwd, segments as _segments, took as _took)  # noqa: F401

pytestmark = pytest.mark.gpu

# per_wave = ceil(kc / 4) selects the instantiation: 1 .. 9, and the looped 10 from kc = 37 (kc = 41: two trips for wave 0)
SPLITK = [(1, 1), (2, 2), (3, 3), (4, 4), (7, 3), (9, 2), (13, 4), (17, 1), (21, 3), (25, 2), (29, 4), (33, 3), (37, 1), (41, 4)]


@pytest.mark.parametrize("M", [37, 160])
@pytest.mark.parametrize("kc,nseg", SPLITK)
def test_forward_split_k(handle, M, kc, nseg):
    i = SPLITK.index((kc, nseg))
    N = (45, 23)[i % 2]
    L = Fwd(1000 + kc, M, _segments(kc, nseg), N)
    assert L.kc == kc and len(L.segs) == nseg
    run_fwd(handle, "fwd split-K kc={} nseg={} M={}".format(kc, nseg, M), L, True, M, (4, 1)[(i + (M == 160)) % 2], "fwd_splitk")


# the smallest shapes the dispatch sends to each family (M, segments, N); the big shapes by pick_big_shape's cost model
THROUGHPUT = [
    ("fwd_t2", 531, ((330, 5, False), (322, 1, False)), 72),    # ragged against 32 rows, 5 column tiles: the last pair is clamped
    ("fwd_rows", 6001, ((13, 5, False), (31, 1, False), (16, 1, True)), 40),   # K = 60 in 4 chunks
    ("fwd_mt", 6001, RICH, 40),
    ("fwd_lds", 65537, RICH, 40),
    ("fwd_big_3x2", 6100, RICH, 256),
    ("fwd_big_4x2", 6400, RICH, 256),
    ("fwd_big_2x2", 8192, RICH, 128),
    ("fwd_big_3x2", 10000, RICH, 128),
    ("fwd_big_3x3", 1920, RICH, 1152),
]


@pytest.mark.parametrize("family,M,segs,N", THROUGHPUT, ids=["{}-{}x{}".format(f, m, n) for f, m, _, n in THROUGHPUT])
def test_forward_throughput_kernels(handle, family, M, segs, N):
    L = Fwd(M + N, M, segs, N)
    case = "fwd {} M={} K={} N={}".format(family, M, L.K, N)
    ref = L.reference(True, M)
    run_fwd(handle, case + " rich out_ld=N+4", L, True, M, 4, family, ref)
    run_fwd(handle, case + " rich out_ld=N+1", L, True, M, 1, family, ref)
    if family.startswith("fwd_big"):   # the vector fast path, with an addend
        run_fwd(handle, case + " plain out_ld=N+4", L, False, M, 4, family)


@pytest.mark.parametrize("N,big,small", [(256, (6400, "fwd_big_4x2"), (6100, "fwd_big_3x2")),
                                         (128, (10000, "fwd_big_3x2"), (8192, "fwd_big_2x2"))])
def test_tile_shape_does_not_change_a_bit(handle, N, big, small):
    """sq_launch_linear / pick_big_shape: every tile shape of k_linear_big accumulates an output in the same order."""
    L = Fwd(7 * N, big[0], RICH, N)
    y_big = run_fwd(handle, "bits N={} M={}".format(N, big[0]), L, False, big[0], 4, big[1])
    y_small = run_fwd(handle, "bits N={} M={}".format(N, small[0]), L, False, small[0], 4, small[1])
    differ = _bits(y_big[:small[0]]) != _bits(y_small)
    assert not differ.any(), "{} of {} outputs differ between {} and {}".format(int(differ.sum()), differ.size, big[1], small[1])


def test_forward_refusals(handle):
    """A segment base off 16 bytes, or a pitch that is no multiple of 4 floats: -5, nothing launched, nothing counted."""
    lib, h = handle
    M, N = 37, 45
    L = Fwd(5, M + 1, RICH, N)
    out = torch.full((M, N + 4), float("nan"), device="cuda")
    for what, kw in (("base", dict(seg_ptr=L.d_x[0].data_ptr() + 4)), ("pitch", dict(seg_ld=L.ld[0] + 1))):
        before = _capi.dense_routes()
        rc = lib.sqair_linear_contract_test(h, C.byref(L.contract(True, M, out, N + 4, **kw)), stream())
        torch.cuda.synchronize()
        assert rc == -5, (what, rc)
        assert b"sqair_linear_contract_test" in lib.sqair_last_error(h)
        assert _took(before) == {}, what
        assert np.isnan(out.cpu().numpy()).all(), what


# ------------------------------------------------------------------------------------------------------------------------------
# dX
# ------------------------------------------------------------------------------------------------------------------------------
SPM_FLOOR = F64(np.float32(1e-2))   # dx_dact's constant is the float32 one


def _dact64(o, act):
    o = o.astype(F64)
    return [np.ones_like(o), np.where(o > 0, 1.0, o + 1.0), 1.0 - o * o, o * (1.0 - o), 1.0 - np.exp(-(o - SPM_FLOOR))][act]


EDGES = {NONE: (0.5, -0.5), ELU: (0.0, -1.0 + 1e-7), TANH: (1.0, -1.0), SIGMOID: (0.0, 1.0), SOFTPLUS_MIN: (1e-2, 1e-2)}


def _saved_output(rng, M, ld, acts):
    """A saved activation OUTPUT [M, ld] whose column c went through acts[c], with the edges of each activation's range in rows
    0, 1 and M - 1 (the last row of a ragged tile)."""
    pre = rng.standard_normal((M, ld))
    out = np.empty((M, ld), np.float32)
    for c in range(ld):
        a = acts[c] if c < len(acts) else NONE
        out[:, c] = act64(pre[:, c], a).astype(np.float32)
        out[0, c], out[1, c], out[M - 1, c] = EDGES[a][0], EDGES[a][1], EDGES[a][c % 2]
    return out


def _dx_bar(width):
    return 2e-5 * max(1.0, np.sqrt(width / 256.0))


def _check_dest(case, name, got, init, M, c0, c1, ref, bar_rel, allowance=0.0, extra=None):
    """`got` against `init` bit for bit outside rows [0, M) x columns [c0, c1); inside, finite and within the bar of `ref`."""
    own = np.zeros(got.shape, bool)
    own[:M, c0:c1] = True
    if extra is not None:
        own |= extra
    changed = (_bits(got) != _bits(init)) & ~own
    assert not changed.any(), "{} {}: {} elements outside the launch's rows and columns changed, first at {}".format(
        case, name, int(changed.sum()), tuple(np.argwhere(changed)[0]))
    g = got[:M, c0:c1]
    assert np.isfinite(g).all(), (case, name)
    mag = float(np.abs(ref).max())
    err = float(np.abs(g.astype(F64) - ref).max()) / max(mag, 1e-30)
    bar = bar_rel + allowance / max(mag, 1e-30)
    print("{} {}: rel err {:.3e} bar {:.3e}".format(case, name, err, bar))
    assert err < bar, (case, name, err, bar)
    return err, bar


class _Dx:
    def __init__(self, seed, M, width, Kdim, pitch=None):
        self.rng = rng = np.random.default_rng(seed)
        self.M, self.width, self.Kdim = M, width, Kdim
        self.ld = pitch or ((width + 3) & ~3) + 4
        self.dpre = rng.standard_normal((M, self.ld)).astype(np.float32)
        self.dpre[:, width:] *= 1e3   # pad columns: finite, and nothing may come of them
        self.w = (rng.standard_normal((Kdim, width)) / np.sqrt(width)).astype(np.float32)
        self.d_dpre, self.d_w = _dev(self.dpre), _dev(self.w)
        kc, nt = (width + 15) // 16, (Kdim + 15) // 16
        self.per_wave = (kc + 3) // 4
        self.scratch = torch.empty(2 * nt * kc * 256 + 256, dtype=torch.float32, device="cuda")
        self.keep = []

    def v(self, scale=1.0):
        return self.dpre[:, :self.width].astype(F64) @ self.w.astype(F64).T * scale

    def args(self, scale_ptr=None):
        t = _capi.SqairDxTest()
        t.dpre, t.ld, t.width, t.M = self.d_dpre.data_ptr(), self.ld, self.width, self.M
        t.w, t.Kdim = self.d_w.data_ptr(), self.Kdim
        t.scale_ptr = scale_ptr
        t.scratch, t.scratch_bytes = self.scratch.data_ptr(), self.scratch.numel() * 4
        return t

    def buffer(self, rows, ld, known):
        """A destination: NaN, or known values where the launch accumulates.  Returns (host copy, device tensor)."""
        init = self.rng.standard_normal((rows, ld)).astype(np.float32) if known else np.full((rows, ld), np.nan, np.float32)
        d = _dev(init)
        self.keep.append(d)
        return init, d


def _three_ranges(D, Kdim):
    """[0, 50) with an ELU / none split at 20 and a second destination; [64, 200) accumulating into its destination, through a
    tanh / sigmoid split; [208, Kdim) with its own addend and a softplus + 0.01 saved output.  Pitches take in the columns up to
    the next range's 16-aligned start (the last one: up to the padded tile edge), so that a write there shows."""
    M, rng = D.M, D.rng
    spec = [dict(n0=0, n1=50, ld=68, dst2=72, add=None, acts=(ELU, NONE, 20)),
            dict(n0=64, n1=200, ld=148, dst2=None, add="dst", acts=(TANH, SIGMOID, 70)),
            dict(n0=208, n1=Kdim, ld=((Kdim + 15) // 16) * 16 - 208 + 4, dst2=None, add="own", acts=(SOFTPLUS_MIN, NONE, 1 << 30))]
    for r in spec:
        n = r["n1"] - r["n0"]
        r["init"], r["d_dst"] = D.buffer(M + 3, r["ld"], r["add"] == "dst")
        if r["dst2"]:
            r["init2"], r["d_dst2"] = D.buffer(M + 3, r["dst2"], False)
        r["saved_ld"] = n + 3
        a, b, split = r["acts"]
        r["saved"] = _saved_output(rng, M, r["saved_ld"], [a if c < split else b for c in range(n)])
        r["d_saved"] = _dev(r["saved"])
        if r["add"] == "own":
            r["add_ld"] = n + 5
            r["addv"] = rng.standard_normal((M, r["add_ld"])).astype(np.float32)
            r["d_add"] = _dev(r["addv"])
    return spec


def _fill_ranges(t, spec):
    t.nranges = len(spec)
    for i, r in enumerate(spec):
        q = t.r[i]
        q.n0, q.n1, q.dst, q.dst_ld = r["n0"], r["n1"], r["d_dst"].data_ptr(), r["ld"]
        if r["dst2"]:
            q.dst2, q.dst2_ld = r["d_dst2"].data_ptr(), r["dst2"]
        if r["add"] == "dst":
            q.add, q.add_ld = r["d_dst"].data_ptr(), r["ld"]
        elif r["add"] == "own":
            q.add, q.add_ld = r["d_add"].data_ptr(), r["add_ld"]
        q.saved, q.saved_ld = r["d_saved"].data_ptr(), r["saved_ld"]
        q.act_a, q.act_b, q.act_split = r["acts"]


def _check_ranges(case, D, spec, v, family):
    worst = (0.0, 1.0)
    for i, r in enumerate(spec):
        n, M = r["n1"] - r["n0"], D.M
        ref = v[:, r["n0"]:r["n1"]].copy()
        if r["add"] == "dst":
            ref += r["init"][:M, :n].astype(F64)
        elif r["add"] == "own":
            ref += r["addv"][:, :n].astype(F64)
        a, b, split = r["acts"]
        c = np.arange(n)
        ref *= np.where(c < split, _dact64(r["saved"][:, :n], a), _dact64(r["saved"][:, :n], b))
        res = [_check_dest(case, "range {} dst".format(i), r["d_dst"].cpu().numpy(), r["init"], M, 0, n, ref, _dx_bar(D.width))]
        if r["dst2"]:
            res.append(_check_dest(case, "range {} dst2".format(i), r["d_dst2"].cpu().numpy(), r["init2"], M, 0, n, ref, _dx_bar(D.width)))
            assert np.array_equal(_bits(r["d_dst2"].cpu().numpy()[:M, :n]), _bits(r["d_dst"].cpu().numpy()[:M, :n]))
        worst = max([worst] + res, key=lambda eb: eb[0] / eb[1])
    dense_record(case, family=family, err=worst[0], bar=worst[1], ratio=worst[0] / worst[1])


NCH_OF = {1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 6: 6, 7: 7, 8: 8, 9: 9, 10: 12, 11: 12, 12: 12}
# width -> per_wave: 1, 4, 9, 10 (<12> with invalid trailing chunks), 13 and 18 (<18>, one trip), 19 (<18> looped, a nearly empty
# second block), 5 with width % 4 != 0 (pitch 312: one finite pad column); the remaining instantiations at 37 rows
PLAIN = [(M, w) for w in (50, 250, 570, 630, 820, 1150, 1204, 311) for M in (37, 160)] + [(37, w) for w in (100, 180, 370, 440, 500)]


@pytest.mark.parametrize("M,width", PLAIN)
def test_dx_ranges(handle, M, width):
    lib, h = handle
    Kdim = 250
    D = _Dx(width * 3 + M, M, width, Kdim, pitch=312 if width == 311 else None)
    family = "dx_nch{}".format(NCH_OF.get(D.per_wave, 18))
    case = "dx ranges M={} width={} (per_wave {})".format(M, width, D.per_wave)
    use_scale = width == 250
    d_scale = _dev(np.array([0.75], np.float32))
    spec = _three_ranges(D, Kdim)
    t = D.args(d_scale.data_ptr() if use_scale else None)
    _fill_ranges(t, spec)
    before = _capi.dense_routes()
    rc = lib.sqair_linear_dx_test(h, C.byref(t), stream())
    assert rc == 0, lib.sqair_last_error(h)
    took = _took(before)
    assert took == {family: 1}, "{}: meant for {}, the launcher took {}".format(case, family, took)
    _check_ranges(case, D, spec, D.v(0.75 if use_scale else 1.0), family)


def test_dx_32x32_tiles(handle):
    lib, h = handle
    M, width, Kdim = 531, 652, 328
    D = _Dx(11, M, width, Kdim)
    case = "dx t2 M={} width={} Kdim={}".format(M, width, Kdim)
    spec = _three_ranges(D, Kdim)
    t = D.args()
    _fill_ranges(t, spec)
    before = _capi.dense_routes()
    rc = lib.sqair_linear_dx_test(h, C.byref(t), stream())
    assert rc == 0, lib.sqair_last_error(h)
    took = _took(before)
    assert took == {"dx_t2": 1}, took
    _check_ranges(case, D, spec, D.v(), "dx_t2")


@pytest.mark.parametrize("M", [37, 160])
@pytest.mark.parametrize("nh", [128, 256])
@pytest.mark.parametrize("mode", [1, 2])
def test_dx_gru_epilogues(handle, mode, nh, M):
    lib, h = handle
    sig = lambda v: (1.0 / (1.0 + np.exp(-v))).astype(np.float32)
    for width in (nh, 50):
        for acc_dh in (0, 1):
            for dup in ("none", "gates", "gates+candidate"):
                D = _Dx(mode * 1000 + nh + M + width + acc_dh, M, width, nh)
                rng = D.rng
                case = "dx gru{} nh={} M={} width={} acc_dh={} dup={}".format(mode, nh, M, width, acc_dh, dup)
                g0_ld, g1_ld, h_ld, dp_ld, dh_ld, dup_ld = nh + 4, nh + 8, nh + 12, 3 * nh + 4, nh + 4, 2 * nh + 12
                dup_h_off = nh + 4 if dup == "gates+candidate" else -1
                g0, g1 = sig(rng.standard_normal((M, g0_ld))), np.tanh(rng.standard_normal((M, g1_ld))).astype(np.float32)
                hp = rng.standard_normal((M, h_ld)).astype(np.float32)
                d_g0, d_g1, d_hp = _dev(g0), _dev(g1), _dev(hp)
                dp_init, d_dp = D.buffer(M + 2, dp_ld, False)
                dh_init, d_dh = D.buffer(M + 2, dh_ld, mode == 2 or acc_dh == 1)
                dup_init, d_dup = D.buffer(M + 2, dup_ld, False)
                t = D.args()
                t.nranges = 1
                t.r[0].n0, t.r[0].n1 = 0, nh
                G = t.gru
                G.mode, G.nh = mode, nh
                G.g0, G.g0_ld, G.g1, G.g1_ld, G.hprev, G.h_ld = d_g0.data_ptr(), g0_ld, d_g1.data_ptr(), g1_ld, d_hp.data_ptr(), h_ld
                G.dpre1, G.dp_ld, G.d_h, G.dh_ld, G.acc_dh = d_dp.data_ptr(), dp_ld, d_dh.data_ptr(), dh_ld, acc_dh
                if dup != "none":
                    G.dup, G.dup_ld = d_dup.data_ptr(), dup_ld
                G.dup_h_off = dup_h_off
                before = _capi.dense_routes()
                rc = lib.sqair_linear_dx_test(h, C.byref(t), stream())
                assert rc == 0, lib.sqair_last_error(h)
                family = "dx_gru{}".format(mode)
                took = _took(before)
                assert took == {family: 1}, "{}: the launcher took {}".format(case, took)

                v = D.v()

                def formulas(g, z_or_r, hc, hprev, dh0):
                    one = g.dtype.type(1)
                    if mode == 1:
                        z = z_or_r
                        return dict(dz=g * (hc - hprev) * z * (one - z), dc=g * z * (one - hc * hc), dh=dh0 + g * (one - z))
                    r = z_or_r
                    return dict(dr=g * hprev * r * (one - r), dh=dh0 + g * r)

                accumulate = mode == 2 or acc_dh == 1
                ops = (g0[:, :nh], g1[:, :nh], hp[:, :nh], dh_init[:M, :nh] if accumulate else np.zeros((M, nh), np.float32))
                ref = formulas(v, *[o.astype(F64) for o in ops])
                f32 = formulas(v.astype(np.float32), *ops)
                allow = {k: 4.0 * float(np.abs(f32[k].astype(F64) - ref[k]).max()) for k in ref}
                bar_rel = _dx_bar(width)
                got_dp, got_dh, got_dup = d_dp.cpu().numpy(), d_dh.cpu().numpy(), d_dup.cpu().numpy()
                res = {}
                if mode == 1:
                    second = np.zeros(got_dp.shape, bool)
                    second[:M, 2 * nh:3 * nh] = True
                    res["dpre1 z"] = _check_dest(case, "dpre1[:, 0:nh]", got_dp, dp_init, M, 0, nh, ref["dz"], bar_rel, allow["dz"], second)
                    first = np.zeros(got_dp.shape, bool)
                    first[:M, :nh] = True
                    res["dpre1 h"] = _check_dest(case, "dpre1[:, 2nh:3nh]", got_dp, dp_init, M, 2 * nh, 3 * nh, ref["dc"], bar_rel, allow["dc"], first)
                    if dup == "none":
                        assert np.array_equal(_bits(got_dup), _bits(dup_init)), case
                    else:
                        cand = np.zeros(got_dup.shape, bool)
                        if dup_h_off >= 0:
                            cand[:M, dup_h_off:dup_h_off + nh] = True
                            gates = np.zeros(got_dup.shape, bool)
                            gates[:M, :nh] = True
                            res["dup h"] = _check_dest(case, "dup[:, off:]", got_dup, dup_init, M, dup_h_off, dup_h_off + nh, ref["dc"], bar_rel, allow["dc"], gates)
                        res["dup z"] = _check_dest(case, "dup[:, 0:nh]", got_dup, dup_init, M, 0, nh, ref["dz"], bar_rel, allow["dz"], cand)
                else:
                    res["dpre1 r"] = _check_dest(case, "dpre1[:, nh:2nh]", got_dp, dp_init, M, nh, 2 * nh, ref["dr"], bar_rel, allow["dr"])
                    if dup == "none":
                        assert np.array_equal(_bits(got_dup), _bits(dup_init)), case
                    else:
                        res["dup r"] = _check_dest(case, "dup[:, 0:nh]", got_dup, dup_init, M, 0, nh, ref["dr"], bar_rel, allow["dr"])
                res["d_h"] = _check_dest(case, "d_h", got_dh, dh_init, M, 0, nh, ref["dh"], bar_rel, allow["dh"])
                k = max(res, key=lambda n: res[n][0] / res[n][1])
                key = {"dpre1 z": "dz", "dup z": "dz", "dpre1 h": "dc", "dup h": "dc", "dpre1 r": "dr", "dup r": "dr", "d_h": "dh"}[k]
                dense_record(case, family=family, destination=k, err=res[k][0], bar=res[k][1], ratio=res[k][0] / res[k][1],
                        f32_formula_err=allow[key] / 4.0, allowance=allow[key])


def test_dx_refusals(handle):
    """A range start off 16 columns: -5.  A GRU block with a saved pointer, with two ranges, or deeper than 16 K chunks on the
    product build: -6.  Nothing launched, nothing counted."""
    lib, h = handle
    M, nh = 37, 128
    D = _Dx(3, M, 50, nh)
    init, d_dst = D.buffer(M, 3 * nh + 4, False)   # (wide enough for whatever a launch that should not happen would write)
    z = _dev(np.full((M, nh), 0.5, np.float32))

    def plain(n0):
        t = D.args()
        t.nranges = 1
        t.r[0].n0, t.r[0].n1, t.r[0].dst, t.r[0].dst_ld = n0, nh, d_dst.data_ptr(), 3 * nh + 4
        return t

    def gru(D=D, saved=False, two=False):
        t = D.args()
        t.nranges = 2 if two else 1
        t.r[0].n0, t.r[0].n1 = 0, nh
        if two:
            t.r[0].n1 = 64
            t.r[1].n0, t.r[1].n1 = 64, nh
        if saved:
            t.r[0].saved, t.r[0].saved_ld = z.data_ptr(), nh
        G = t.gru
        G.mode, G.nh, G.dup_h_off = 1, nh, -1
        G.g0 = G.g1 = G.hprev = z.data_ptr()
        G.g0_ld = G.g1_ld = G.h_ld = nh
        G.dpre1, G.dp_ld, G.d_h, G.dh_ld = d_dst.data_ptr(), 3 * nh + 4, d_dst.data_ptr(), 3 * nh + 4
        return t

    deep = _Dx(4, M, 300, nh)   # 19 K chunks: per_wave 5
    for what, t, want in (("n0 % 16", plain(8), -5), ("gru + saved", gru(saved=True), -6), ("gru + two ranges", gru(two=True), -6),
                          ("gru per_wave > 4", gru(D=deep), -6)):
        before = _capi.dense_routes()
        rc = lib.sqair_linear_dx_test(h, C.byref(t), stream())
        torch.cuda.synchronize()
        assert rc == want, (what, rc)
        assert b"sqair_linear_dx_test" in lib.sqair_last_error(h), what
        assert _took(before) == {}, what
        assert np.array_equal(_bits(d_dst.cpu().numpy()), _bits(init)), what
