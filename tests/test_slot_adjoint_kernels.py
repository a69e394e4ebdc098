"""-m gpu: the element-wise adjoints of the slot loop, each on its own against float64 autograd.

k_slot_tail_bwd, k_crop_chain_bwd<staged | LDS-DMA>, k_where_param_grads and k_gru_bwd_a / _b run through their unit entries
(sqair_slot_tail_bwd_test, sqair_crop_chain_bwd_test, sqair_where_param_grads_test, sqair_gru_gates_bwd_test: the launchers of
sqair_backward on caller-owned buffers) and are compared with tests/slot_adjoint_ref.py -- the forward of each piece restated on the
oracle's functions, differentiated by autograd, pinned on the CPU by tests/test_slot_adjoint_ref.py.

Inputs.  The tape (saved activations, records) is drawn in float64, rounded to float32, and given as the same float32 values to the
kernel and to the reference; upstream gradients are random, of mixed sign and magnitude (N(0, 1) x 10^U(-2, 1)).  Every operand with a
pitch has one wider than its width; what a kernel must not read is NaN (padding, the other slots, phases and record fields, every
parameter but the ones the launch is about), what it must not write holds distinct words and is compared bit for bit afterwards;
accumulated outputs (d_rec_prev, d_mask, flat_grad) start from known non-zero content; second copies (d_s1pre2, dup_z, dup_r) are
compared bit for bit with the first.

Where logits of the crop cases are drawn per row by rejection on the REFERENCE's margin: a row is redrawn until every sampling
coordinate of its glimpse is at least 1e-3 pixel from an integer (the kink of bilinear sampling, where fp32 and fp64 may take
different taps).  Nothing is selected on a kernel's result, and no row is left out of a comparison.

Metric and bars.  An element's error is divided by the largest magnitude of the reference in its row (a where quadruple, the n_what
entries, the hidden units, a glimpse), for the twelve reduced scalars by the float64 sum of the absolute terms.  The bar of a (kernel,
output) is 8 x the worst error, in the same metric over the kernel's cases, of the SAME reference evaluated in float32 on the CPU
(8 ulp of the row scale where that is exactly zero).  With SQAIR_PARITY_DIR set the figures go to slot_adjoint_parity.json there (the
copy under profiles/ is such a file).

A glimpse wholly outside the frame does not exist under to_coords (the shift is a tanh: the glimpse's centre is inside the frame);
the cases put saturated shifts and large scales in their first rows, which leaves most of those glimpses outside."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from sqair_amd import _capi
from tests import kernel_unit as U
from tests import slot_adjoint_ref as R
from tests.hip_util import stream
from tests.kernel_unit import CHOLESKY, F32, F64, SCALE_OFFSET, Buf, pitched, records
from tests.kernel_unit import f32 as _f32, image as _image, mixed as _mixed

pytestmark = pytest.mark.gpu

KINK = 1e-3


# ------------------------------------------------------------------------------------------------ handles
HANDLES = {   # name: (wide, (H, W), N, K, flags)
    "t_50_256": (False, (50, 50), 4, 1, dict()),
    "t_7_128": (False, (50, 50), 3, 1, dict(n_what=7, n_units=4)),
    "t_50_128": (False, (50, 50), 4, 1, dict(n_units=4)),
    "t_128_256_wide": (True, (50, 50), 3, 1, dict(n_what=128)),
    "t_50_512_wide": (True, (50, 50), 3, 1, dict(n_units=16)),
    "n1": (False, (50, 50), 1, 1, dict()),
    "c_50x50": (False, (50, 50), 4, 3, dict()),
    "c_64x64_g12": (False, (64, 64), 3, 2, dict(glimpse_size=12)),
    "c_65x64": (False, (65, 64), 3, 3, dict()),
    "c_128x128": (False, (128, 128), 3, 2, dict()),
    "c_33x48_g12": (False, (33, 48), 3, 3, dict(glimpse_size=12)),
    "c_33x47_g12": (False, (33, 47), 3, 3, dict(glimpse_size=12)),
    "c_50x50_g36": (False, (50, 50), 3, 3, dict(glimpse_size=36)),
    "c_50x50_512_wide": (True, (50, 50), 3, 3, dict(n_units=16)),
}


def handle(name):
    return U.handle(name, lambda n: U.Handle(n, *HANDLES[n]))


PARITY = U.Parity("slot_adjoint_parity.json",
                  "per case of tests/test_slot_adjoint_kernels.py and output: the kernel's largest row-scaled error against float64 "
                  "autograd, the bar (8 x the worst error of the same reference in float32 over the kernel's cases), the float32 "
                  "reference's own error in this case; `bars`: per kernel and output the float32 figure the bar comes from")
_cases = U.Cases(lambda kernel: {k: BUILD[kernel](*v) for k, v in CASES[kernel].items()})


def _worst32(kernel):
    """Per output: the worst row-scaled error of the fp32 reference over all cases of the kernel."""
    return U.worst32(_cases(kernel))


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    U.close()
    PARITY.write(_worst32)


def _judge(kernel, case, got, c, scales=None):
    assert set(got) == set(c["ref"])
    U.judge(PARITY, kernel, case, got, lambda k: R.row_scaled_error(got[k], c["ref"][k], (scales or {}).get(k)), c["err32"], _worst32(kernel))


# ------------------------------------------------------------------------------------------------ slot tail
TAIL_CASES = {   # name: (handle, is_disc, slot, R, enc_pre, second copy of d_s1pre, seed)
    "disc slot0 R18 pre": ("t_50_256", 1, 0, 18, 1, 0, 1),
    "disc slot2 R40 post": ("t_50_256", 1, 2, 40, 0, 0, 2),
    "disc slot3 R1 pre": ("t_50_256", 1, 3, 1, 1, 0, 3),
    "prop slot0 R40 copy": ("t_50_256", 0, 0, 40, 0, 1, 4),
    "prop slot2 R18": ("t_50_256", 0, 2, 18, 0, 0, 5),
    "prop slot3 R1 copy": ("t_50_256", 0, 3, 1, 0, 1, 6),
    "disc slot1 R18 pre nw7 nh128": ("t_7_128", 1, 1, 18, 1, 0, 7),
    "prop slot2 R40 copy nw7 nh128": ("t_7_128", 0, 2, 40, 0, 1, 8),
    "disc slot0 R40 post nw50 nh128": ("t_50_128", 1, 0, 40, 0, 0, 9),
    "prop slot3 R18 nw50 nh128": ("t_50_128", 0, 3, 18, 0, 0, 10),
    "wide disc slot1 R18 pre nw128": ("t_128_256_wide", 1, 1, 18, 1, 0, 11),
    "wide prop slot2 R18 copy nw128": ("t_128_256_wide", 0, 2, 18, 0, 1, 12),
    "wide disc slot0 R18 pre nh512": ("t_50_512_wide", 1, 0, 18, 1, 0, 13),
    "wide prop slot1 R40 copy nh512": ("t_50_512_wide", 0, 1, 40, 0, 1, 14),
}
HRAW_BLOCKS = ("loc", "scale", "fg", "ig", "tg")


def _tail_outputs(g, content, nw, dtype):
    """The reference's outputs in the kernel's units; accumulated ones include the known content (added in `dtype`)."""
    o = dict(d_s1pre=g["d_s1pre"], d_raw=g["d_raw"][:, None], d_what=g["d_what"], d_enc_loc=g["d_enc"][:, :nw], d_enc_scale=g["d_enc"][:, nw:])
    if "d_hraw" in g:
        for i, k in enumerate(HRAW_BLOCKS):                                   # what-head loc, raw scale, the three raw gates
            o["d_hraw_" + k] = g["d_hraw"][:, i * nw:(i + 1) * nw]
        o["d_what_tm1"] = (content.astype(dtype) + g["d_what_tm1"].astype(dtype))
    return {k: np.asarray(v, F64) for k, v in o.items()}


def build_tail(hname, is_disc, slot, R_, enc_pre, copy, seed):
    wide, _, N, _, flags = HANDLES[hname]
    nw, nh = flags.get("n_what", 50), 32 * flags.get("n_units", 8)
    nsp = nh // 2
    rng = np.random.default_rng(1000 + seed)
    prev = (rng.uniform(size=R_) < 0.6).astype(F32)
    prev[0] = 1.0
    if R_ > 1:
        prev[1] = 0.0
    if is_disc and slot == 0:
        prev[:] = 1.0                                   # (taken without a read)
    consts = dict(eps=_f32(rng.standard_normal((R_, nw))), w_what=_f32(rng.standard_normal((nw, nsp)) * 0.4 / np.sqrt(nw)),
                  w2=_f32(rng.standard_normal(nsp) / np.sqrt(nsp)), b2=F32(0.25), prev=prev, is_disc=bool(is_disc))
    enc_raw = rng.uniform(-12.0, 3.0, size=(R_, nw))                                      # scales down to the 0.01 floor
    enc = _f32(np.concatenate([rng.standard_normal((R_, nw)), (O.softplus(torch.as_tensor(enc_raw)) + 1e-2).numpy()], -1))
    s1h = _f32(O.elu(torch.as_tensor(rng.standard_normal((R_, nsp)) * 1.5)).numpy())     # both signs
    tape = dict(enc=enc, s1h=s1h, hraw=None, what_tm1=None)
    if not is_disc:
        # a third of the gates out to +-12, the others N(0, 1.5), and one per row and gate that is surely not saturated: a row of
        # saturated gates only has no scale to measure against but the rounding of 1 - sigmoid (in any fp32 evaluation)
        gates = np.where(rng.uniform(size=(R_, 3, nw)) < 0.33, rng.uniform(-12, 12, size=(R_, 3, nw)), rng.standard_normal((R_, 3, nw)) * 1.5)
        gates[:, :, 0] = rng.uniform(-1, 1, size=(R_, 3))
        tape["hraw"] = _f32(np.concatenate([rng.standard_normal((R_, nw)), rng.uniform(-12, 3, size=(R_, nw)), gates.reshape(R_, 3 * nw)], -1))
        tape["what_tm1"] = _f32(rng.standard_normal((R_, nw)))
    up = dict(what=_mixed(rng, (R_, nw)), what_loc=_mixed(rng, (R_, nw)), what_scale=_mixed(rng, (R_, nw)), logit=_mixed(rng, (R_,)))
    content = _f32(rng.standard_normal((R_, nw)) * 3.0)                                   # what d_rec_prev[WHAT] already holds
    ref = {}
    for dt, tdt in ((F64, torch.float64), (F32, torch.float32)):
        ref[dt] = _tail_outputs(R.tail_adjoint(tape, consts, up, tdt, enc_pre=bool(enc_pre)), content, nw, dt)
    assert all(v.shape[0] == R_ for v in ref[F64].values())                              # every row is compared
    scales = {}
    if enc_pre:
        # The gradient of the what head's PRE-activation is d scale x softplus'(raw), and the kernel has only the saved scale to get
        # softplus' from: 1 - exp(-(scale - 0.01)), a difference of two terms of size 1 that cancels at the 0.01 floor (raw -12:
        # 6e-6 left of 1).  Whatever rounds the exponential to fp32 leaves half an ulp of 1 there, times d scale: an ill-conditioned
        # quantity, judged on the size of its terms: the row's largest |d scale| instead of the row's largest product.  (Measured
        # in the product's own scale the kernel is at 4.3e-6 in the n_what = 7 case against 8 x 4.6e-7 of the fp32 reference, which
        # differentiates softplus at the inverted raw value and has no such difference; in the terms' scale it is at 8e-8.)
        for dt, tdt in ((F64, torch.float64), (F32, torch.float32)):
            ref[dt]["d_enc_scale_pre"] = ref[dt].pop("d_enc_scale")
        d_scale = R.tail_adjoint(tape, consts, up, torch.float64, enc_pre=False)["d_enc"][:, nw:]
        scales["d_enc_scale_pre"] = np.abs(d_scale).max(-1, keepdims=True)
        assert np.all(scales["d_enc_scale_pre"] >= np.abs(ref[F64]["d_enc_scale_pre"]).max(-1, keepdims=True))
    return dict(args=(hname, is_disc, slot, R_, enc_pre, copy), consts=consts, tape=tape, up=up, content=content, ref=ref[F64], scales=scales,
                err32={k: R.row_scaled_error(ref[F32][k], ref[F64][k], scales.get(k)) for k in ref[F64]}, nw=nw, nsp=nsp)


def run_tail(case_name, c):
    hname, is_disc, slot, R_, enc_pre, copy = c["args"]
    hd = handle(hname)
    L, N, W, nw, nsp = hd.L, hd.N, hd.L["W"], c["nw"], c["nsp"]
    assert nw == hd.nw and nsp == hd.nh // 2
    phase = 1 if is_disc else 0
    core = "disc" if is_disc else "prop"
    # parameters: everything NaN but the steps predictor's output weights and the `what` rows of its hidden layer
    # (oracle: features [hidden | what] in discovery, [hidden | temporal state | what] in propagation)
    flat = np.full(L["n_flat"], np.nan, F32)
    o, n = hd.off[core + ".steps.l1.w"]
    assert n == nsp
    flat[o:o + nsp] = c["consts"]["w2"]
    o, n = hd.off[core + ".steps.l0.w"]
    first = (1 if is_disc else 2) * hd.nh
    assert n == (first + nw) * nsp
    flat[o + first * nsp:o + n] = c["consts"]["w_what"].reshape(-1)
    rec_new, rec_prev = records(R_, N, W, "nan"), records(R_, N, W, "nan")
    if is_disc and slot > 0:
        rec_new[:, slot - 1, L["PRES"]] = c["consts"]["prev"]
    if not is_disc:
        rec_prev[:, slot, L["PRES"]] = c["consts"]["prev"]
        rec_prev[:, slot, L["WHAT"]:L["WHAT"] + nw] = c["tape"]["what_tm1"]
    d_new, d_prev = records(R_, N, W, 0), records(R_, N, W, R_ * N * W)
    d_new[:, slot, L["LOGIT"]] = c["up"]["logit"]
    for col, k in (("WHAT", "what"), ("WHAT_LOC", "what_loc"), ("WHAT_SCALE", "what_scale")):
        d_new[:, slot, L[col]:L[col] + nw] = c["up"][k]
    own_new, own_prev = np.zeros(d_new.shape, bool), np.zeros(d_prev.shape, bool)
    own_new[:, slot, L["WHAT"]:L["WHAT"] + nw] = True
    if not is_disc:
        d_prev[:, slot, L["WHAT"]:L["WHAT"] + nw] = c["content"]
        own_prev[:, slot, L["WHAT"]:L["WHAT"] + nw] = True
    noise = np.full((R_, 2, N, hd.nzw), np.nan, F32)
    noise[:, phase, slot, 4:4 + nw] = c["consts"]["eps"]
    B = dict(flat=Buf(flat), rec_new=Buf(rec_new), rec_prev=Buf(rec_prev), d_new=Buf(d_new, own_new), d_prev=Buf(d_prev, own_prev), noise=Buf(noise))
    at = 2 * R_ * N * W
    t = _capi.SqairSlotTailBwdTest()
    t.is_disc, t.slot, t.B, t.enc_pre = is_disc, slot, R_, enc_pre
    t.rec_prev, t.rec_new, t.d_rec_new, t.d_rec_prev = B["rec_prev"].ptr(), B["rec_new"].ptr(), B["d_new"].ptr(), B["d_prev"].ptr()
    t.noise, t.flat = B["noise"].ptr(), B["flat"].ptr()
    B["s1h"], t.s1h = pitched(R_, nsp, nsp + 8, c["tape"]["s1h"]); t.s1h_ld = nsp + 8
    B["enc"], t.enc = pitched(R_, 2 * nw, 2 * nw + 5, c["tape"]["enc"]); t.enc_ld = 2 * nw + 5
    for name, width, ld, field, ldf in (("d_s1pre", nsp, nsp + 4, "d_s1pre", "ds_ld"), ("d_raw", 1, 3, "d_raw_out", "dr_ld"),
                                        ("d_enc", 2 * nw, 2 * nw + 7, "d_enc", "de_ld")):
        B[name], p = pitched(R_, width, ld, out=True, start=at); at += B[name].before.size
        setattr(t, field, p); setattr(t, ldf, ld)
    if copy:
        B["d_s1pre2"], t.d_s1pre2 = pitched(R_, nsp, nsp + 12, out=True, start=at); at += B["d_s1pre2"].before.size
        t.ds2_ld = nsp + 12
    if not is_disc:
        B["hraw"], t.hraw = pitched(R_, 5 * nw, 5 * nw + 3, c["tape"]["hraw"]); t.h_ld = 5 * nw + 3
        B["d_hraw"], t.d_hraw = pitched(R_, 5 * nw, 5 * nw + 9, out=True, start=at); t.dh_ld = 5 * nw + 9
    hd.check(hd.lib.sqair_slot_tail_bwd_test(hd.h, C.byref(t), stream()), "sqair_slot_tail_bwd_test")
    for name, b in B.items():
        b.check_untouched(name)
    view = lambda n: B[n].p.view(B[n].after())
    got = dict(d_s1pre=view("d_s1pre"), d_raw=view("d_raw"), d_what=B["d_new"].after()[:, slot, L["WHAT"]:L["WHAT"] + nw],
               d_enc_loc=view("d_enc")[:, :nw], d_enc_scale=view("d_enc")[:, nw:])
    if not is_disc:
        for i, k in enumerate(HRAW_BLOCKS):
            got["d_hraw_" + k] = view("d_hraw")[:, i * nw:(i + 1) * nw]
        got["d_what_tm1"] = B["d_prev"].after()[:, slot, L["WHAT"]:L["WHAT"] + nw]
    if copy:
        assert np.array_equal(view("d_s1pre2").view(np.uint32), view("d_s1pre").view(np.uint32)), "d_s1pre2 is not a copy of d_s1pre"
    if enc_pre:
        got["d_enc_scale_pre"] = got.pop("d_enc_scale")
    _judge("slot_tail", case_name, got, c, c["scales"])


@pytest.mark.parametrize("case", sorted(TAIL_CASES))
def test_slot_tail_adjoint(case):
    run_tail(case, _cases("slot_tail")[case])


# ------------------------------------------------------------------------------------------------ crop chain
CROP_CASES = {}   # name: (handle, B, mode, slot, mask: 0 none / 1 present / 2 present with the fused sigmoid adjoint, fuse_t3, seed)
for _i, (_h, _B) in enumerate([("c_50x50", 3), ("c_64x64_g12", 8), ("c_65x64", 3), ("c_128x128", 8), ("c_33x48_g12", 3), ("c_33x47_g12", 3),
                               ("c_50x50_g36", 3)]):
    _N = HANDLES[_h][2]
    _s = 20 * _i
    CROP_CASES[_h + " prop1 mask+dact"] = (_h, _B, 1, 0, 2, 0, _s + 1)
    CROP_CASES[_h + " prop2 slot%d mask fused" % (_N - 1)] = (_h, _B, 2, _N - 1, 1, 1, _s + 2)
    CROP_CASES[_h + " disc slot1"] = (_h, _B, 3, 1, 0, 0, _s + 3)
CROP_CASES.update({
    "c_50x50 prop1 no mask": ("c_50x50", 3, 1, 0, 0, 0, 4),
    "c_50x50 prop1 mask": ("c_50x50", 3, 1, 0, 1, 0, 5),
    "c_50x50 prop2 slot0 mask": ("c_50x50", 3, 2, 0, 1, 0, 6),
    "c_50x50 disc slot0 fused": ("c_50x50", 3, 3, 0, 0, 1, 7),
    "c_50x50_512_wide prop2 slot1 mask fused": ("c_50x50_512_wide", 3, 2, 1, 1, 1, 8),
    "c_50x50_512_wide disc slot2 fused": ("c_50x50_512_wide", 3, 3, 2, 0, 1, 9),
    "c_50x50_512_wide prop1 mask+dact": ("c_50x50_512_wide", 3, 1, 0, 2, 0, 10),
})

def _draw_where(rng, rows, H, W, G):
    """Where logits per row, redrawn until the reference's kink margin holds; the first rows saturate the shift / take a large
    scale (most of those glimpses lie outside the frame).  Returns (logits fp32, share of rows that passed at the first draw)."""
    def draw(n):
        w = rng.standard_normal((n, 4)) * np.array([1.0, 1.0, 0.8, 0.8]) + np.array([-0.5, -0.5, 0.0, 0.0])
        return w.astype(F32)
    w = draw(rows)
    special = np.array([[2.0, 1.5, 12.0, -12.0], [3.0, 3.0, -2.5, 2.5], [-1.0, 2.0, 4.0, 0.3]], F32)
    k = min(rows, len(special))
    w[:k] = special[:k]
    first = None
    for _ in range(200):
        bad = R.kink_margin(w, H, W, G) < KINK
        first = 1.0 - bad.mean() if first is None else first
        if not bad.any():
            return w, float(first)
        fresh = draw(int(bad.sum()))
        keep_special = np.flatnonzero(bad) < k                     # a special row is nudged, not replaced
        fresh[keep_special] = w[bad][keep_special] + rng.uniform(-0.05, 0.05, size=(int(keep_special.sum()), 4)).astype(F32)
        w[bad] = fresh
    raise AssertionError("no kink-free where draw")


def build_crop(hname, B_, mode, slot, mask_mode, fuse, seed):
    wide, (H, W), N, K, flags = HANDLES[hname]
    G, nh = flags.get("glimpse_size", 20), 32 * flags.get("n_units", 8)
    G2, R_ = G * G, B_ * K
    rng = np.random.default_rng(5000 + seed)
    rows = R_ * N if mode == 1 else R_
    img = _image(rng, B_, H, W)
    frame_of = np.repeat(np.arange(B_), K)                                   # row r reads frame r // K
    img_rows = img[np.repeat(frame_of, N) if mode == 1 else frame_of]
    consts = dict(img=img_rows, G=G, mode=mode)
    tape = dict(mask=None)
    if mode == 1:
        wb = _f32(rng.standard_normal((rows, 4)))
        wl, first = _draw_where(rng, rows, H, W, G)
        where_tm1 = _f32(wl.astype(F64) - 0.1 * wb.astype(F64))
        for _ in range(200):   # the margin is the REFERENCE's, on the logits it forms from the fp32 operands
            bad = R.kink_margin(where_tm1.astype(F64) + 0.1 * wb.astype(F64), H, W, G) < KINK
            if not bad.any():
                break
            where_tm1[bad] += rng.uniform(-0.02, 0.02, size=(int(bad.sum()), 4)).astype(F32)
        wl64 = where_tm1.astype(F64) + 0.1 * wb.astype(F64)
        tape.update(wb=wb, where_tm1=where_tm1)
    else:
        where, first = _draw_where(rng, rows, H, W, G)
        wl64 = where.astype(F64)
        tp = _f32(rng.standard_normal((rows, 8)) * np.array([1, 1, 1, 1, 2.5, 2.5, 2.5, 2.5]))
        eps = _f32(rng.standard_normal((rows, 4)))
        consts.update(scale_offset=SCALE_OFFSET[mode], eps=eps, cholesky=CHOLESKY, w3=_f32(rng.standard_normal((nh, 8)) * 0.3))
        # the record's loc / the transform output consistent with the saved where (to rounding)
        cc = {k: (v if isinstance(v, int) else torch.as_tensor(np.asarray(v, F64))) for k, v in consts.items()}
        o = R.crop_forward(dict(tp=torch.as_tensor(tp.astype(F64)), where_tm1=torch.zeros(rows, 4, dtype=torch.float64),
                                bump=torch.zeros(rows, 4, dtype=torch.float64)), cc)
        shift = where.astype(F64) - o["where"].numpy()
        if mode == 2:
            tape["where_tm1"] = _f32(shift)
        else:
            tp[:, :4] = _f32(tp[:, :4] + shift)
        t2 = np.where(rng.uniform(size=(rows, nh)) < 0.5, rng.uniform(0.05, 2.0, size=(rows, nh)), -rng.uniform(0.02, 0.98, size=(rows, nh)))
        tape.update(tp=tp, where=where, t2=_f32(t2))
    margin = R.kink_margin(wl64, H, W, G)
    assert margin.shape == (rows,) and margin.min() >= KINK                 # every row kept, every row stable
    if mask_mode:
        m = rng.uniform(0.02, 0.98, size=(rows, G2))
        m[:, [0, G - 1, G2 - G, G2 - 1]] = rng.choice([1e-6, 1.0 - 1e-6, 0.5], size=(rows, 4))   # the glimpse's corner pixels
        tape["mask"] = _f32(m)
    up = dict(glimpse=_mixed(rng, (rows, G2)))
    if mode != 1:
        up.update(where=_mixed(rng, (rows, 4)), where_loc=_mixed(rng, (rows, 4)), where_scale=_mixed(rng, (rows, 4)))
    if mask_mode:
        up["mask"] = _f32(rng.standard_normal((rows, G2)) * 2.0)            # what d_mask already holds
    content = _f32(rng.standard_normal((rows, 4)) * 3.0)                    # what d_rec_prev[WHERE] already holds
    ref = {}
    for dt, tdt in ((F64, torch.float64), (F32, torch.float32)):
        g = R.crop_adjoint(tape, consts, up, tdt, fuse_t3=bool(fuse), mask_dact=mask_mode == 2)
        o = {}
        if mode == 1:
            o["d_wb"] = g["d_wb"]
        else:
            o.update(d_tp_loc=g["d_tp"][:, :4], d_tp_raw=g["d_tp"][:, 4:], d_where=g["d_where"])
            if fuse:
                o["d_t2"] = g["d_t2"]
        if mode != 3:
            o["d_where_tm1"] = content.astype(dt) + g["d_where_tm1"].astype(dt)
        if mask_mode:
            o["d_mask"] = g["d_mask"]
        ref[dt] = {k: np.asarray(v, F64) for k, v in o.items()}
    assert all(v.shape[0] == rows for v in ref[F64].values())
    return dict(args=(hname, B_, mode, slot, mask_mode, fuse), img=img, consts=consts, tape=tape, up=up, content=content, ref=ref[F64],
                err32={k: R.row_scaled_error(ref[F32][k], ref[F64][k]) for k in ref[F64]}, first_pass=first, rows=rows)


def run_crop(case_name, c):
    hname, B_, mode, slot, mask_mode, fuse = c["args"]
    hd = handle(hname)
    L, N, K, W_, G2, nh = hd.L, hd.N, hd.K, hd.L["W"], hd.G * hd.G, hd.nh
    H, Wd = hd.hw
    R_, rows = B_ * K, c["rows"]
    P, P4 = H * Wd, (H * Wd + 3) // 4 * 4
    frames = np.zeros((B_, P4), F32)                                         # each frame zero-padded to a multiple of 4 floats
    frames[:, :P] = c["img"].reshape(B_, P)
    flat = np.full(L["n_flat"], np.nan, F32)
    if mode != 1:
        core = "prop" if mode == 2 else "disc"
        flat[hd.off[core + ".transform.scale_offset"][0]] = SCALE_OFFSET[mode]
        if mode == 2:
            o, n = hd.off["prop.cholesky_scale"]
            assert n == 10
            flat[o:o + 10] = CHOLESKY
    rec_new, rec_prev = records(R_, N, W_, "nan"), records(R_, N, W_, "nan")
    d_new, d_prev = records(R_, N, W_, 0), records(R_, N, W_, R_ * N * W_)
    own_new, own_prev = np.zeros(d_new.shape, bool), np.zeros(d_prev.shape, bool)
    wh = slice(L["WHERE"], L["WHERE"] + 4)
    if mode == 1:
        rec_prev[:, :, wh] = c["tape"]["where_tm1"].reshape(R_, N, 4)
        d_prev[:, :, wh] = c["content"].reshape(R_, N, 4)
        own_prev[:, :, wh] = True
    else:
        rec_new[:, slot, wh] = c["tape"]["where"]
        for col, k in (("WHERE", "where"), ("WHERE_LOC", "where_loc"), ("WHERE_SCALE", "where_scale")):
            d_new[:, slot, L[col]:L[col] + 4] = c["up"][k]
        own_new[:, slot, wh] = True
        d_prev[:, slot, wh] = c["content"]
        own_prev[:, slot, wh] = mode == 2                                    # (discovery reads it and leaves it alone)
    noise = np.full((R_, 2, N, hd.nzw), np.nan, F32)
    if mode != 1:
        noise[:, 1 if mode == 3 else 0, slot, 0:4] = c["consts"]["eps"]
    B = dict(img=Buf(frames), flat=Buf(flat), rec_new=Buf(rec_new), rec_prev=Buf(rec_prev), d_new=Buf(d_new, own_new), d_prev=Buf(d_prev, own_prev),
             noise=Buf(noise))
    at = 2 * R_ * N * W_
    t = _capi.SqairCropChainBwdTest()
    t.mode, t.slot, t.B, t.mask_dact = mode, (0 if mode == 1 else slot), B_, int(mask_mode == 2)
    t.img, t.flat, t.noise = B["img"].ptr(), B["flat"].ptr(), B["noise"].ptr()
    t.rec_prev, t.rec_new, t.d_rec_prev, t.d_rec_new = B["rec_prev"].ptr(), B["rec_new"].ptr(), B["d_prev"].ptr(), B["d_new"].ptr()
    # glimpse gradients and masks live in row-pitched buffers: row r (and slot k of crop #1) at r * mul + add (+ k)
    g_mul, g_add = (N, 0) if mode == 1 else (2, 1)
    m_mul, m_add = N + 1, (0 if mode == 1 else slot)
    per = N if mode == 1 else 1
    def scatter(data, mul, add, fill):
        a = np.full((R_ * mul + add + 1, G2), np.nan, F32) if fill == "nan" else R.distinct_words((R_ * mul + add + 1) * G2, fill).reshape(-1, G2).copy()
        idx = (np.arange(R_)[:, None] * mul + add + np.arange(per)[None, :]).reshape(-1)
        a[idx] = data
        return a, idx
    g_host, _ = scatter(c["up"]["glimpse"], g_mul, g_add, "nan")
    B["g_out"] = Buf(g_host)
    t.g_out, t.g_row_mul, t.g_row_add = B["g_out"].ptr(), g_mul, g_add
    if mask_mode:
        m_host, midx = scatter(c["tape"]["mask"], m_mul, m_add, "nan")
        dm_host, _ = scatter(c["up"]["mask"], m_mul, m_add, at); at += dm_host.size
        own = np.zeros(dm_host.shape, bool)
        own[midx] = True
        B["mask"], B["d_mask"] = Buf(m_host), Buf(dm_host, own)
        t.mask, t.d_mask, t.mask_row_mul, t.mask_row_add = B["mask"].ptr(), B["d_mask"].ptr(), m_mul, m_add
    if mode == 1:
        B["wb"], t.wb = pitched(rows, 4, 6, c["tape"]["wb"]); t.wb_ld = 6
        B["d_wb"], t.d_wb = pitched(rows, 4, 6, out=True, start=at)          # (one pitch for both: CropChainBwdArgs has one wb_ld)
    else:
        B["tp"], t.tp = pitched(R_, 8, 9, c["tape"]["tp"]); t.tp_ld = 9
        B["d_tp"], t.d_tp = pitched(R_, 8, 11, out=True, start=at); t.dtp_ld = 11; at += B["d_tp"].before.size
        if fuse:
            B["w3"] = Buf(c["consts"]["w3"])
            B["t2"], t.t2 = pitched(R_, nh, nh + 1, c["tape"]["t2"]); t.t2_ld = nh + 1
            B["d_t2"], t.d_t2 = pitched(R_, nh, nh + 4, out=True, start=at); t.dt2_ld = nh + 4
            t.w3 = B["w3"].ptr()
    hd.check(hd.lib.sqair_crop_chain_bwd_test(hd.h, C.byref(t), stream()), "sqair_crop_chain_bwd_test")
    for name, b in B.items():
        b.check_untouched(name)
    view = lambda n: B[n].p.view(B[n].after())
    got = {}
    if mode == 1:
        got["d_wb"] = view("d_wb")
        got["d_where_tm1"] = B["d_prev"].after()[:, :, wh].reshape(rows, 4)
    else:
        got.update(d_tp_loc=view("d_tp")[:, :4], d_tp_raw=view("d_tp")[:, 4:], d_where=B["d_new"].after()[:, slot, wh])
        if mode == 2:
            got["d_where_tm1"] = B["d_prev"].after()[:, slot, wh]
        if fuse:
            got["d_t2"] = view("d_t2")
    if mask_mode:
        got["d_mask"] = B["d_mask"].after()[midx]
    assert all(v.shape[0] == rows for v in got.values())
    _judge("crop_chain", case_name, got, c)


@pytest.mark.parametrize("case", sorted(CROP_CASES))
def test_crop_chain_adjoint(case):
    c = _cases("crop_chain")[case]
    print("{}: {:.0%} of the rows' where draws passed the kink margin first time".format(case, c["first_pass"]))
    run_crop(case, c)


def test_crop_chain_instantiation_boundary():
    """4096 pixels is the last frame the LDS-staged instantiation takes, the next shape the first of the LDS-DMA one; both are among the
    cases above.  (The staged kernel's loop over 'frames beyond 4096 pixels' is therefore never entered: DESIGN.md section 9.)"""
    assert HANDLES["c_64x64_g12"][1] == (64, 64) and 64 * 64 == 4096
    assert HANDLES["c_65x64"][1] == (65, 64) and 65 * 64 > 4096
    assert (33 * 47) % 4 != 0 and (33 * 48) % 4 == 0


# ------------------------------------------------------------------------------------------------ where parameters
WPG_CASES = {"T1 R1 N1": ("n1", 1, 1, 1), "T1 R37 N1": ("n1", 1, 37, 2), "T3 R700 N4": ("t_50_256", 3, 700, 3)}   # (handle, T, B = R, seed)


def build_wpg(hname, T_, R_, seed):
    N = HANDLES[hname][2]
    rows = T_ * R_ * N
    rng = np.random.default_rng(9000 + seed)
    x = dict(d_where=_mixed(rng, (rows, 4)), scale=_f32(rng.uniform(0.011, 1.5, size=(rows, 4))), eps=_f32(rng.standard_normal((rows, 4))),
             d_raw_p=_mixed(rng, (rows, 4)), d_raw_d=_mixed(rng, (rows, 4)))
    content = _f32(rng.standard_normal(12) * 2.0)
    g64, tot = R.where_param_adjoint(x["d_where"], x["scale"], x["eps"], x["d_raw_p"], x["d_raw_d"], torch.float64, with_abs=True)
    g32 = R.where_param_adjoint(x["d_where"], x["scale"], x["eps"], x["d_raw_p"], x["d_raw_d"], torch.float32)
    ref64 = content.astype(F64) + g64
    ref32 = (content + g32.astype(F32)).astype(F64)
    scale = tot + np.abs(content.astype(F64))                               # the sum of the absolute terms, the content among them
    return dict(args=(hname, T_, R_), x=x, content=content, ref=dict(twelve=ref64), scale=scale, rows=rows,
                err32=dict(twelve=R.row_scaled_error(ref32, ref64, scale)))


def _run_wpg(hd, T_, R_, x, content):
    L, N, W_ = hd.L, hd.N, hd.L["W"]
    rows = T_ * R_ * N
    d_rec, rec = np.full((rows, W_), np.nan, F32), np.full((rows, W_), np.nan, F32)
    d_rec[:, L["WHERE"]:L["WHERE"] + 4] = x["d_where"]
    rec[:, L["WHERE_SCALE"]:L["WHERE_SCALE"] + 4] = x["scale"]
    noise = np.full((T_, R_, 2, N, hd.nzw), np.nan, F32)
    noise[:, :, 0, :, 0:4] = x["eps"].reshape(T_, R_, N, 4)
    d_tp = np.full((2 * rows, 8), np.nan, F32)                               # (columns 0:4, the loc half, are not this kernel's)
    d_tp[:rows, 4:], d_tp[rows:, 4:] = x["d_raw_p"], x["d_raw_d"]
    grad = R.distinct_words(L["n_flat"], 7).copy()
    idx = np.concatenate([hd.off["prop.cholesky_scale"][0] + np.arange(10), [hd.off["prop.transform.scale_offset"][0]],
                          [hd.off["disc.transform.scale_offset"][0]]])
    grad[idx] = content
    own = np.zeros(grad.shape, bool)
    own[idx] = True
    B = dict(d_rec=Buf(d_rec), rec=Buf(rec), noise=Buf(noise), grad=Buf(grad, own))
    t = _capi.SqairWhereParamGradsTest()
    B["d_tp"], t.d_tp = pitched(2 * rows, 8, 9, d_tp); t.tp_ld = 9
    t.T, t.B, t.d_rec_p, t.rec_p, t.noise, t.flat_grad = T_, R_, B["d_rec"].ptr(), B["rec"].ptr(), B["noise"].ptr(), B["grad"].ptr()
    hd.check(hd.lib.sqair_where_param_grads_test(hd.h, C.byref(t), stream()), "sqair_where_param_grads_test")
    for name, b in B.items():
        b.check_untouched(name)
    return B["grad"].after()[idx]


@pytest.mark.parametrize("case", sorted(WPG_CASES))
def test_where_param_grads(case):
    c = _cases("where_param_grads")[case]
    hname, T_, R_ = c["args"]
    got = _run_wpg(handle(hname), T_, R_, c["x"], c["content"])
    assert c["rows"] == {"T1 R1 N1": 1, "T1 R37 N1": 37, "T3 R700 N4": 8400}[case]      # (8400: beyond the launch's 8192 threads)
    _judge("where_param_grads", case, dict(twelve=got), c, dict(twelve=c["scale"]))


def test_where_param_grads_cholesky_order():
    """One use, one non-zero d where_i, one non-zero eps_j: the product lands in the entry of prop.cholesky_scale that
    oracle.fill_triangular puts at (i, j) of the factor -- exactly (2 x 0.5 x 3), on zero content, nothing else touched."""
    hd = handle("n1")
    order = O.fill_triangular(torch.arange(1.0, 11.0, dtype=torch.float64), 4).numpy()
    for i in range(4):
        for j in range(i + 1):
            x = dict(d_where=np.zeros((1, 4), F32), scale=np.full((1, 4), 0.5, F32), eps=np.zeros((1, 4), F32), d_raw_p=np.zeros((1, 4), F32),
                     d_raw_d=np.zeros((1, 4), F32))
            x["d_where"][0, i], x["eps"][0, j] = 2.0, 3.0
            want = np.zeros(12, F32)
            want[int(order[i, j]) - 1] = 3.0
            got = _run_wpg(hd, 1, 1, x, np.zeros(12, F32))
            assert np.array_equal(got, want), (i, j, got.tolist())


# ------------------------------------------------------------------------------------------------ GRU gates
GRU_CASES = {   # name: (handle, rows, broadcast h, accumulate_dh, dup: 0 none / 1 gates (dup_h_off -1) / 2 gates + candidate at 2 nh, seed)
    "nh256 rows1 bcast acc0 dup0": ("t_50_256", 1, 1, 0, 0, 1),
    "nh256 rows18 pitch acc1 dup2": ("t_50_256", 18, 0, 1, 2, 2),
    "nh256 rows160 bcast acc0 dup1": ("t_50_256", 160, 1, 0, 1, 3),
    "nh256 rows160 pitch acc1 dup0": ("t_50_256", 160, 0, 1, 0, 4),
    "nh128 rows1 pitch acc1 dup1": ("t_50_128", 1, 0, 1, 1, 5),
    "nh128 rows18 bcast acc0 dup2": ("t_50_128", 18, 1, 0, 2, 6),
    "nh128 rows160 pitch acc0 dup2": ("t_50_128", 160, 0, 0, 2, 7),
}


def build_gru(hname, rows, bcast, acc, dup, seed):
    nh = 32 * HANDLES[hname][4].get("n_units", 8)
    rng = np.random.default_rng(7000 + seed)
    def gate(fn):
        a = rng.uniform(-12, 12, size=(rows, nh))
        y = _f32(fn(torch.as_tensor(a)).numpy())
        sat = rng.uniform(size=(rows, nh))
        y[sat < 0.02] = 1.0                                                  # saturated on both sides, exactly
        y[sat > 0.98] = -1.0 if fn is torch.tanh else 0.0
        return y
    tape = dict(z=gate(torch.sigmoid), r=gate(torch.sigmoid), hc=gate(torch.tanh), h=_f32(rng.standard_normal((1 if bcast else rows, nh))))
    up = dict(h_new=_mixed(rng, (rows, nh)), rh=_mixed(rng, (rows, nh)))
    content = _f32(rng.standard_normal((rows, nh)) * 2.0)
    ref = {}
    for dt, tdt in ((F64, torch.float64), (F32, torch.float32)):
        g = R.gru_adjoint(tape, up, tdt)
        dh = g["d_h_a"].astype(dt) + g["d_h_b"].astype(dt)
        if acc:
            dh = (content.astype(dt) + g["d_h_a"].astype(dt)) + g["d_h_b"].astype(dt)
        ref[dt] = {k: np.asarray(v, F64) for k, v in dict(d_az=g["d_az"], d_ar=g["d_ar"], d_ah=g["d_ah"], d_h=dh).items()}
    return dict(args=(hname, rows, bcast, acc, dup), tape=tape, up=up, content=content, ref=ref[F64], nh=nh,
                err32={k: R.row_scaled_error(ref[F32][k], ref[F64][k]) for k in ref[F64]})


@pytest.mark.parametrize("case", sorted(GRU_CASES))
def test_gru_gate_adjoints(case):
    c = _cases("gru_gates")[case]
    hname, rows, bcast, acc, dup = c["args"]
    hd, nh = handle(hname), c["nh"]
    assert hd.nh == nh
    t = _capi.SqairGruGatesBwdTest()
    t.rows, t.accumulate_dh = rows, acc
    B = {}
    for name, field, ldf, ld in (("z", "z", "z_ld", nh + 4), ("r", "r", "r_ld", nh + 8), ("hc", "hc", "hc_ld", nh + 12)):
        B[name], p = pitched(rows, nh, ld, c["tape"][name]); setattr(t, field, p); setattr(t, ldf, ld)
    B["d_hn"], t.d_hn = pitched(rows, nh, nh + 3, c["up"]["h_new"]); t.dhn_ld = nh + 3
    B["d_rh"], t.d_rh = pitched(rows, nh, nh + 5, c["up"]["rh"]); t.drh_ld = nh + 5
    if bcast:
        B["h"], t.hprev = pitched(1, nh, nh, c["tape"]["h"]); t.h_ld = 0
    else:
        B["h"], t.hprev = pitched(rows, nh, nh + 7, c["tape"]["h"]); t.h_ld = nh + 7
    at = 0
    B["dpre1"], t.dpre1 = pitched(rows, 3 * nh, 3 * nh + 4, out=True, start=at); t.dp_ld = 3 * nh + 4; at += B["dpre1"].before.size
    # d_h: an output that starts from known content (accumulate_dh 1 adds to it, 0 overwrites it)
    p = R.Pitched(rows, nh, nh + 2, data=c["content"], nan=False, start=at); at += p.host.size
    own = np.zeros(p.host.shape, bool); own[1:1 + rows, :nh] = True
    B["d_h"] = Buf(p.host, own); B["d_h"].p = p
    t.d_h, t.dh_ld = B["d_h"].ptr(p.first_word()), nh + 2
    t.dup_h_off = -1
    if dup:
        cols = np.ones(3 * nh, bool)
        cols[nh:2 * nh] = False                                              # the r block of the copy is stage B's own buffer
        if dup == 1:
            cols[2 * nh:] = False
        B["dup_z"], t.dup_z = pitched(rows, 3 * nh, 3 * nh + 8, out=True, start=at, owned_cols=cols); at += B["dup_z"].before.size
        t.dupz_ld, t.dup_h_off = 3 * nh + 8, (2 * nh if dup == 2 else -1)
        B["dup_r"], t.dup_r = pitched(rows, nh, nh + 6, out=True, start=at); t.dupr_ld = nh + 6
    hd.check(hd.lib.sqair_gru_gates_bwd_test(hd.h, C.byref(t), stream()), "sqair_gru_gates_bwd_test")
    for name, b in B.items():
        b.check_untouched(name)
    view = lambda n: B[n].p.view(B[n].after())
    d = view("dpre1")
    got = dict(d_az=d[:, :nh], d_ar=d[:, nh:2 * nh], d_ah=d[:, 2 * nh:], d_h=view("d_h"))
    if dup:
        bits = U.bits
        assert np.array_equal(bits(view("dup_z")[:, :nh]), bits(got["d_az"])) and np.array_equal(bits(view("dup_r")), bits(got["d_ar"]))
        if dup == 2:
            assert np.array_equal(bits(view("dup_z")[:, 2 * nh:]), bits(got["d_ah"]))
    _judge("gru_gates", case, got, c)


CASES = dict(slot_tail=TAIL_CASES, crop_chain=CROP_CASES, where_param_grads=WPG_CASES, gru_gates=GRU_CASES)
BUILD = dict(slot_tail=build_tail, crop_chain=build_crop, where_param_grads=build_wpg, gru_gates=build_gru)
