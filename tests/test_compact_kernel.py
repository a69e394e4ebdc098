"""-m gpu: the slot compaction (k_compact) and its adjoint (k_compact_bwd) on their own, every presence pattern against numpy.

The end-to-end suites reach compaction almost only as the identity on the propagated slots (tests/presence_patterns.py says why).
Here the kernels run through `sqair_compact_test` / `sqair_compact_bwd_test` on raw buffers: one particle row per pattern of
(propagated bits x discovered bits), every word of every record, state and initial-state parameter a DISTINCT value, so that one
misrouted 16-byte unit shows.  The forward is a gather: every output is compared bit for bit.  The adjoint copies, adds once
(bit-identical to fp32) or sums up to N terms (judged against the fp64 sum at the bound of an N-term fp32 sum).

Instantiations: the generic k_compact<false>, the specialised k_compact<true> (the shipped shape: sqair_glue.h sq_spec_ok), the wide
library's (another record, plain-loop adjoint); GRU / GRU and LSTM / LSTM state widths; an n_units that is padded."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from tests.hip_util import stream
from tests.kernel_unit import LAYOUT

pytestmark = pytest.mark.gpu

LSTM = dict(time_transition="LSTM", prior_transition="LSTM")
HIDDEN = ("what", "what_loc", "what_scale", "where", "where_loc", "where_scale", "presence_prob", "presence", "presence_logit", "obj_id")


class _Handle:
    def __init__(self, N, wide=False, hw=(50, 50), **flags):
        self.lib = _capi.lib(_capi.WIDE_LIB_PATH if wide else _capi.LIB_PATH)
        self.F = make_flags(k_particles=1, n_steps_per_image=N, **flags)
        cfg = make_config(self.F, hw)
        self.h = C.c_void_p()
        assert self.lib.sqair_create(C.byref(cfg), C.byref(self.h)) == 0
        buf = (C.c_int32 * 20)()
        assert self.lib.sqair_compact_test_layout(self.h, buf, 20) == 20
        self.L = dict(zip(LAYOUT, [int(v) for v in buf]))
        assert self.L["N"] == N and self.L["W"] % 4 == 0 and self.L["snh"] % 4 == 0 and self.L["psnh"] % 4 == 0
        assert 0 <= self.L["temporal_init"] <= self.L["n_flat"] - self.L["snh"]
        assert 0 <= self.L["prior_init"] <= self.L["n_flat"] - self.L["psnh"]

    def close(self):
        self.lib.sqair_destroy(self.h)


def _patterns(N, rng):
    """[rows, 2N] of 0 / 1: propagated bits ++ discovered bits, every pattern in at least two rows."""
    if N <= 4:
        bits = np.array(list(itertools.product((0, 1), repeat=2 * N)), np.float32)          # all 4^N, non-prefix discoveries included
    else:
        bits = (rng.uniform(size=(4096, 2 * N)) < rng.uniform(0.15, 0.85, size=(4096, 1))).astype(np.float32)
        alt = (np.arange(2 * N) % 2).astype(np.float32)
        bits = np.concatenate([bits, np.zeros((1, 2 * N), np.float32), np.ones((1, 2 * N), np.float32), alt[None], 1 - alt[None]])
    bits = np.concatenate([bits, bits[::-1]])                                               # twice, at different row indices
    pad = (-len(bits)) % 8
    return np.concatenate([bits, bits[:pad]]) if pad else bits


def _distinct(shape, start):
    """float32 tensor whose words are consecutive bit patterns from 1.0f upwards: all finite, normal, pairwise distinct."""
    n = int(np.prod(shape))
    assert start + n < (0x7F000000 - 0x3F800000)
    return (np.arange(start, start + n, dtype=np.uint32) + np.uint32(0x3F800000)).view(np.float32).reshape(shape), start + n


def _inputs(hd, bits, seed):
    L, N, R = hd.L, hd.L["N"], len(bits)
    rng = np.random.default_rng(seed)
    x, at = {}, 0
    for k in ("rec_p", "rec_d", "rec_prev"):
        x[k], at = _distinct((R, N, L["W"]), at)
    x["temporal_p"], at = _distinct((R, N, L["snh"]), at)
    x["prior_p"], at = _distinct((R, N, L["psnh"]), at)
    x["flat"], at = _distinct((L["n_flat"],), at)
    x["rec_p"][..., L["PRES"]] = bits[:, :N]
    x["rec_d"][..., L["PRES"]] = bits[:, N:]
    # ids of the previous frame: distinct per slot and row (integers: the id arithmetic is then exact in fp32); last_id above them
    x["rec_prev"][..., L["ID"]] = (rng.integers(0, 1000, size=(R, 1)) + np.arange(N)[None]).astype(np.float32)
    x["last_id_prev"] = (x["rec_prev"][..., L["ID"]].max(-1) + rng.integers(0, 50, size=R)).astype(np.float32)
    return x


def _reference_forward(hd, x, bits):
    """compute_object_ids + select_present on [propagated ++ discovered] in plain numpy."""
    L, N, R = hd.L, hd.L["N"], len(bits)
    src = np.argsort(1.0 - bits, axis=1, kind="stable")[:, :N]
    p, dp = bits[:, :N], bits[:, N:]
    ids = np.concatenate([x["rec_prev"][..., L["ID"]] * p - (1.0 - p),
                          (np.cumsum(dp, 1, dtype=np.float32) + x["last_id_prev"][:, None]) * dp - (1.0 - dp)], 1).astype(np.float32)
    take = lambda a: np.take_along_axis(a, src[:, :, None], 1)
    rec = take(np.concatenate([x["rec_p"], x["rec_d"]], 1))
    rec[..., L["ID"]] = np.take_along_axis(ids, src, 1)
    init = lambda off, w: np.broadcast_to(x["flat"][off:off + w], (R, N, w))
    want = dict(rec_next=rec, src_out=src.astype(np.int32),
                temporal_next=take(np.concatenate([x["temporal_p"], init(L["temporal_init"], L["snh"])], 1)),
                prior_next=take(np.concatenate([x["prior_p"], init(L["prior_init"], L["psnh"])], 1)),
                last_id_next=(x["last_id_prev"] + dp.sum(1, dtype=np.float32)).astype(np.float32))
    nw = L["nw"]
    col = lambda c, w: rec[..., L[c]:L[c] + w]
    want.update(what=col("WHAT", nw), what_loc=col("WHAT_LOC", nw), what_scale=col("WHAT_SCALE", nw), where=col("WHERE", 4),
                where_loc=col("WHERE_LOC", 4), where_scale=col("WHERE_SCALE", 4), presence_prob=rec[..., L["PROB"]],
                presence=rec[..., L["PRES"]], presence_logit=rec[..., L["LOGIT"]], obj_id=rec[..., L["ID"]],
                num_steps_per_sample=rec[..., L["PRES"]].sum(-1, dtype=np.float32))
    return want


SENTINEL = np.float32(-12345.5)


def _run_forward(hd, x, T=2, t=1):
    """Launches k_compact for frame index t of [T]-frame output tensors; every output starts as SENTINEL and has one guard row."""
    L, N, R = hd.L, hd.L["N"], len(x["last_id_prev"])
    dv = {k: torch.as_tensor(v).cuda() for k, v in x.items()}
    full = lambda *shape: torch.full(shape, float(SENTINEL), dtype=torch.float32, device="cuda")
    out = dict(rec_next=full(R + 1, N, L["W"]), temporal_next=full(R + 1, N, L["snh"]), prior_next=full(R + 1, N, L["psnh"]),
               last_id_next=full(R + 1), src_out=torch.full((R + 1, N), -7, dtype=torch.int32, device="cuda"))
    width = dict(what=L["nw"], what_loc=L["nw"], what_scale=L["nw"], where=4, where_loc=4, where_scale=4)
    hid = {k: full(T, R, N, width[k]) if k in width else full(T, R, N) for k in HIDDEN}
    hid["num_steps_per_sample"] = full(T, R)
    so = _capi.SqairOutputs()
    for k, v in hid.items():
        setattr(so, k, v.data_ptr())
    ins = [dv[k].data_ptr() for k in ("rec_p", "rec_d", "rec_prev", "temporal_p", "prior_p", "last_id_prev", "flat")]
    outs = [out[k].data_ptr() for k in ("rec_next", "temporal_next", "prior_next", "last_id_next", "src_out")]
    rc = hd.lib.sqair_compact_test(hd.h, *ins, *outs, C.byref(so), t, R, stream())
    assert rc == 0, hd.lib.sqair_last_error(hd.h)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k, v in got.items():   # the guard row: the launch covers R rows, not one more
        assert (v[R:] == (-7 if k == "src_out" else SENTINEL)).all(), "write beyond the last row of " + k
        got[k] = v[:R]
    for k, v in hid.items():
        a = v.cpu().numpy()
        assert (np.delete(a, t, 0) == SENTINEL).all(), "write outside frame {} of {}".format(t, k)
        got[k] = a[t]
    return got


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def _check_forward(hd, seed=0):
    bits = _patterns(hd.L["N"], np.random.default_rng(seed))
    x = _inputs(hd, bits, seed)
    want = _reference_forward(hd, x, bits)
    got = _run_forward(hd, x)
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        same = _bits(g) == _bits(np.ascontiguousarray(w))
        assert same.all(), "{}: {} of {} words differ, first at {} (pattern {})".format(
            k, int((~same).sum()), same.size, tuple(np.argwhere(~same)[0]), bits[np.argwhere(~same)[0][0]].astype(int).tolist())
    moved = int((want["src_out"][:, :hd.L["N"]] != np.arange(hd.L["N"])[None]).any(1).sum())
    print("k_compact N={} rows={} (rows with a non-identity selection: {}) snh={} psnh={} W={}: bit-identical".format(
        hd.L["N"], len(bits), moved, hd.L["snh"], hd.L["psnh"], hd.L["W"]))
    assert moved >= len(bits) // 4
    return bits, x, got


def _check_adjoint(hd, bits, src, seed=0):
    """k_compact_bwd with `src` from the forward run."""
    L, N, R = hd.L, hd.L["N"], len(bits)
    rng = np.random.default_rng(1000 + seed)
    f = lambda *s: (rng.standard_normal(s) * np.exp(rng.uniform(-3, 3, size=s))).astype(np.float32)   # mixed magnitudes: sums round
    g_rec, g_tmp, g_pri = f(R, N, L["W"]), f(R, N, L["snh"]), f(R, N, L["psnh"])
    pre_p, pre_d = f(R, N, L["W"]), f(R, N, L["W"])          # the kernel ACCUMULATES into the gradient records
    dv = lambda a: torch.as_tensor(a).cuda()
    d_rec_p, d_rec_d = dv(pre_p), dv(pre_d)
    full = lambda *shape: torch.full(shape, float(SENTINEL), dtype=torch.float32, device="cuda")
    d_tmp, d_pri = full(R + 1, N, L["snh"]), full(R + 1, N, L["psnh"])
    d_nt, d_np = full(R + 1, L["snh"]), full(R + 1, L["psnh"])
    ins = [dv(src.astype(np.int32)), dv(g_rec), dv(g_tmp), dv(g_pri)]
    rc = hd.lib.sqair_compact_bwd_test(hd.h, *[t.data_ptr() for t in ins], d_rec_p.data_ptr(), d_rec_d.data_ptr(), d_tmp.data_ptr(),
                                       d_pri.data_ptr(), d_nt.data_ptr(), d_np.data_ptr(), R, stream())
    assert rc == 0, hd.lib.sqair_last_error(hd.h)
    torch.cuda.synchronize()
    # reference: inv[r, sl] = destination of source slot sl, or -1
    inv = np.full((R, 2 * N), -1, np.int64)
    np.put_along_axis(inv, src.astype(np.int64), np.broadcast_to(np.arange(N), (R, N)), 1)
    has = inv >= 0
    gather = lambda g, idx: np.take_along_axis(g, np.maximum(idx, 0)[:, :, None], 1)
    # (1) gradient records: ONE fp32 addition where a merged slot came from the slot, untouched otherwise
    got_rec = np.concatenate([d_rec_p.cpu().numpy(), d_rec_d.cpu().numpy()], 1)
    pre = np.concatenate([pre_p, pre_d], 1)
    want_rec = np.where(has[:, :, None], pre + gather(g_rec, inv), pre).astype(np.float32)
    assert (_bits(got_rec) == _bits(want_rec)).all(), "d_rec_p / d_rec_d"
    assert (_bits(got_rec)[~has] == _bits(pre)[~has]).all(), "a slot no merged slot came from must keep its pre-filled gradient record"
    # (2) recurrent states of the propagated slots: a copy, or exact zeros
    for name, got, g in (("d_temporal_p", d_tmp, g_tmp), ("d_prior_p", d_pri, g_pri)):
        a = got.cpu().numpy()
        assert (a[R:] == SENTINEL).all(), "write beyond the last row of " + name
        want = np.where(has[:, :N, None], gather(g, inv[:, :N]), np.float32(0.0)).astype(np.float32)
        assert (_bits(a[:R]) == _bits(want)).all(), name
        assert (_bits(a[:R])[~has[:, :N]] == 0).all(), name + ": a dropped slot must receive exact zeros"
    # (3) the trainable initial states: up to N terms per element, against the fp64 sum.  A sum of n fp32 terms in any order is
    # within (n - 1) u sum|terms| (1 + O(u)) of the exact one, u = 2^-24: the bar is N u sum|terms|.
    for name, got, g in (("d_new_temporal", d_nt, g_tmp), ("d_new_prior", d_np, g_pri)):
        a = got.cpu().numpy()
        assert (a[R:] == SENTINEL).all(), "write beyond the last row of " + name
        terms = np.where(has[:, N:, None], gather(g, inv[:, N:]), 0.0).astype(np.float64)
        want, mag = terms.sum(1), np.abs(terms).sum(1)
        err = np.abs(a[:R].astype(np.float64) - want)
        bound = N * 2.0 ** -24 * mag
        assert (err <= bound).all(), (name, float((err - bound).max()))
        assert (a[:R][~has[:, N:].any(1)] == 0).all(), name + ": no discovery survived, the sum is empty"
        one = has[:, N:].sum(1) == 1
        assert (_bits(a[:R][one]) == _bits(want[one].astype(np.float32))).all(), name + ": a single term is a copy"
    print("k_compact_bwd N={} rows={}: records / states bit-identical, initial-state sums within N u sum|terms|".format(N, R))


CASES = [
    # id, wide, N, flags, want specialised
    ("n1", False, 1, {}, False),
    ("n2", False, 2, {}, False),
    ("n3", False, 3, {}, False),
    ("n4-specialised", False, 4, {}, True),
    ("n4-generic", False, 4, {"_specialised": 0}, False),
    ("n3-lstm", False, 3, LSTM, False),
    ("n4-lstm", False, 4, LSTM, False),
    ("n2-padded-units", False, 2, dict(n_units=5, **LSTM), False),
    ("n3-padded-units-gru", False, 3, dict(n_units=3), False),
    ("n6", False, 6, dict(n_units=4), False),
    ("n8", False, 8, {}, False),
    ("n8-lstm", False, 8, LSTM, False),   # N snh / 4 = 1024: the last unit of the adjoint's register tiling
    ("wide-n3-what64", True, 3, dict(n_what=64), False),
    ("wide-n2-lstm-units12", True, 2, dict(n_units=12, **LSTM), False),
    ("wide-n4-shipped-shape", True, 4, {}, False),
    ("wide-n8", True, 8, dict(n_units=4), False),
    ("wide-n14", True, 14, dict(n_units=4, n_what=100), False),
]


@pytest.mark.parametrize("wide,N,flags,spec", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_compaction_and_its_adjoint_on_every_presence_pattern(wide, N, flags, spec):
    flags = dict(flags)
    specialised = flags.pop("_specialised", 1)
    hd = _Handle(N, wide=wide, **flags)
    try:
        assert hd.lib.sqair_set_option(hd.h, b"specialised", specialised) == 0
        assert N <= hd.L["max_slots"]
        before = hd.lib.sqair_debug_specialised_launches()
        bits, x, got = _check_forward(hd, seed=N)
        # which instantiation ran is part of the case: k_compact<true> only for the shipped shape with the option on
        took = hd.lib.sqair_debug_specialised_launches() - before
        assert took == (1 if spec else 0), "specialised launches: {}".format(took)
        assert bool(hd.L["spec_ok"]) == (spec or (N == 4 and not flags and not wide))
        _check_adjoint(hd, bits, got["src_out"], seed=N)
    finally:
        hd.close()


def test_specialised_and_generic_compaction_agree_bit_for_bit():
    """The same inputs through k_compact<true> and k_compact<false> (the shipped shape, option on / off)."""
    res = []
    for on in (1, 0):
        hd = _Handle(4)
        try:
            assert hd.lib.sqair_set_option(hd.h, b"specialised", on) == 0
            bits = _patterns(4, np.random.default_rng(0))
            res.append(_run_forward(hd, _inputs(hd, bits, 3)))
        finally:
            hd.close()
    for k in res[0]:
        assert np.array_equal(_bits(res[0][k]), _bits(res[1][k])), k


def test_adjoint_entry_refuses_a_src_that_is_not_a_selection():
    """`src` indexes LDS inside k_compact_bwd: the test entry checks it on the host and launches nothing."""
    hd = _Handle(3)
    try:
        L, N, R = hd.L, 3, 8
        z = lambda *s: torch.zeros(s, device="cuda")
        bufs = [z(R, N, L["W"]), z(R, N, L["snh"]), z(R, N, L["psnh"]), z(R, N, L["W"]), z(R, N, L["W"]), z(R, N, L["snh"]),
                z(R, N, L["psnh"]), z(R, L["snh"]), z(R, L["psnh"])]
        for bad in ([0, 1, 6], [0, 0, 1], [-1, 1, 2]):
            src = torch.tensor([[0, 1, 2]] * (R - 1) + [bad], dtype=torch.int32, device="cuda")
            rc = hd.lib.sqair_compact_bwd_test(hd.h, src.data_ptr(), *[b.data_ptr() for b in bufs], R, stream())
            assert rc == -1 and b"not a slot selection" in hd.lib.sqair_last_error(hd.h)
    finally:
        hd.close()
