"""-m gpu: the SMC resampler kernel (k_smc_resample, through sqair_smc_resample_test) against the float64 resampler of
tests/smc_ref.py, on caller buffers: K in {1, 2, 63, 64, 65, 255, 256} (one wave, a wave boundary, several waves per lane),
T in {1, 4}, thousands of lanes with weight patterns where fp32 goes wrong, ess_frac in {0, 1e-3, 0.5, 1}, caller uniforms and
Philox.

Tolerances come from fp32 rounding of the header's formula, per lane (smc_ref.rounding_band: the error of the fixed-order sums
of e_k = expf(a_k - m)), and are capped at 1e-5 relative.  A decision or a threshold inside that band is skipped and counted; at
most 10 % of them may be."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from tests import smc_ref as S

pytestmark = pytest.mark.gpu

U = S.FP32_EPS
CAP = 1e-5
PATTERNS = ("random", "equal", "dominant", "spread", "huge", "neg_inf", "u_zero", "u_top")
SEED = (1 << 32) + 77


def _lanes(K, T, lanes_per_pattern, rng):
    """lw0 [B*K], lw [T, B*K], log_z [B], caller u [B], pattern name per lane, plus one NaN lane and one all -inf lane."""
    L = lanes_per_pattern
    B = L * len(PATTERNS) + 2
    lw0 = np.zeros((B, K), np.float32)
    lw = np.zeros((T, B, K), np.float32)
    u = rng.uniform(size=B).astype(np.float32)
    names = []
    for p, name in enumerate(PATTERNS):
        sl = slice(p * L, (p + 1) * L)
        names += [name] * L
        if name in ("random", "u_zero", "u_top"):
            lw0[sl] = rng.standard_normal((L, K)) * 2
            lw[:, sl] = rng.standard_normal((T, L, K)) * 3
        elif name == "equal":        # ESS = K exactly; at u = 0 the ties give the identity
            lw0[sl] = rng.standard_normal((L, 1)) * 5
            lw[:, sl] = rng.standard_normal((T, L, 1))
        elif name == "dominant":     # ESS = 1 exactly: the others underflow (-inf in half the lanes)
            lw0[sl] = np.where((np.arange(L) % 2 == 0)[:, None], -np.inf, -200.0)
            lw0[np.arange(p * L, (p + 1) * L), rng.integers(0, K, L)] = 0.0   # (anywhere: rarely the last particle)
        elif name == "spread":       # 80-110 nats: expf underflows at the bottom
            span = rng.uniform(80, 110, size=(L, 1))
            lw0[sl] = -rng.uniform(size=(L, K)) * span
        elif name == "huge":         # magnitudes ~1e5 (the fp32 ulp is 8e-3 there)
            lw0[sl] = 1e5 * np.where(np.arange(L)[:, None] % 2 == 0, 1.0, -1.0) + rng.standard_normal((L, K))
            lw[:, sl] = rng.standard_normal((T, L, K))
        elif name == "neg_inf":      # some particles at -inf: never chosen
            lw0[sl] = rng.standard_normal((L, K))
            dead = rng.uniform(size=(L, K)) < 0.4
            dead[:, 0] = False   # (one alive per lane: a lane all at -inf is the non-finite case below)
            lw0[sl] = np.where(dead, -np.inf, lw0[sl])
        if name in ("u_zero", "equal"):
            u[sl] = 0.0
        if name in ("u_top", "dominant"):
            u[sl] = np.float32(1.0 - 2.0 ** -24)
    lw0[-2, K // 2] = np.nan            # a NaN lane
    lw0[-1, :] = -np.inf                # an all -inf lane
    names += ["nan", "all_neg_inf"]
    R = B * K
    return B, lw0.reshape(R), lw.reshape(T, R), rng.standard_normal(B).astype(np.float32), u, names


def _band_Q(w, K):
    """rounding_band for sum e_k^2: a -> 2a and m -> 2m double e_k's subtraction term, as squaring does (the squaring's own
    rounding and the second expf ulp are added by the caller)."""
    from types import SimpleNamespace
    return S.rounding_band(SimpleNamespace(a=2 * w.a, m=2 * w.m, e=w.e * w.e), K)


def _thr32(u, S32, K):
    """The kernel's thresholds fl(fl(fl(k + u) S) / K) in fp32."""
    k = np.arange(K, dtype=np.float32)
    return (((k + np.float32(u)).astype(np.float32) * np.float32(S32)).astype(np.float32) / np.float32(K)).astype(np.float64)


def _run(lib, h, lw0, lw, log_z, T, B, K, frac, uniforms, t_row):
    dev = lambda x, dt=torch.float32: torch.as_tensor(np.ascontiguousarray(x), dtype=dt).cuda()
    d = dict(lw=dev(lw), log_w=dev(lw0), log_z=dev(log_z), log_evidence=torch.zeros(B, device="cuda"),
             ess=torch.zeros(B, device="cuda"), u_out=torch.full((B,), -1.0, device="cuda"),
             resampled=torch.full((B,), -7, dtype=torch.int32, device="cuda"),
             src=torch.full((B * K,), -7, dtype=torch.int32, device="cuda"), t_row=dev(t_row, torch.int32))
    uni = dev(uniforms) if uniforms is not None else None
    smc = _capi.SqairSmc(ess_frac=frac, seed=SEED, uniforms=uni.data_ptr() if uni is not None else None,
                         log_w=d["log_w"].data_ptr(), log_z=d["log_z"].data_ptr(), log_evidence=d["log_evidence"].data_ptr(),
                         ess=d["ess"].data_ptr(), u_out=d["u_out"].data_ptr(), resampled=d["resampled"].data_ptr(),
                         src_rows=d["src"].data_ptr())
    s = torch.cuda.current_stream()
    rc = lib.sqair_smc_resample_test(h, d["lw"].data_ptr(), T, B, K, d["t_row"].data_ptr(), C.byref(smc), C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in d.items()}


@pytest.fixture(scope="module")
def handle():
    lib = _capi.lib()
    cfg = make_config(make_flags(k_particles=2, n_steps_per_image=3), (50, 50))
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    lib.sqair_destroy(h)


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 255, 256])
@pytest.mark.parametrize("T", [1, 4])
def test_resampler_kernel_against_fp64(handle, K, T):
    lib, h = handle
    rng = np.random.default_rng(1000 * K + T)
    L = max(8, 4096 // (K * len(PATTERNS)) + 8)   # a few thousand lanes at small K, >= 8 per pattern at large K
    B, lw0, lw, log_z, u_caller, names = _lanes(K, T, L, rng)
    t_row = np.repeat(rng.integers(0, 1 << 20, B), K).astype(np.int32)
    counts = dict(dec_checked=0, dec_skipped=0, anc_checked=0, anc_skipped=0, went=0)
    for frac in (0.0, 1e-3, 0.5, 1.0):
        for caller in (True, False):
            got = _run(lib, h, lw0, lw, log_z, T, B, K, frac, u_caller if caller else None, t_row)
            if caller:
                u = u_caller
                assert np.array_equal(got["u_out"], u_caller)
            else:   # Philox keyed by (seed, lane, counter of row b*K after the pass): bit for bit
                u = S.smc_uniform(np.arange(B), t_row[::K] + T, SEED)
                assert np.array_equal(got["u_out"], u), np.argwhere(got["u_out"] != u)[:4]
            ref = S.resample(lw0, lw, log_z, u, K, frac)
            w = ref.w
            fin = np.isfinite(ref.ess)
            assert np.array_equal(fin, np.isfinite(got["ess"])), np.flatnonzero(fin != np.isfinite(got["ess"]))
            assert not fin[-2:].any() and fin[:-2].all()
            # ESS: |error| <= 2 rel(S) + rel(Q) + 3u (product, quotient, squares) + 2 ulp (expf in e^2), capped at 1e-5 relative
            bS = S.rounding_band(w, K)
            bQ = _band_Q(w, K)
            Q = (w.e * w.e).sum(1)
            with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
                tol_ess = np.minimum(2 * bS / w.S + bQ / Q + 4 * U + 2 * S.ULP2, CAP)
                # where S and Q lie farther than their bands from an fp32 rounding boundary, the device's sums ARE fl(S) and
                # fl(Q), and its ESS is fl(fl(S^2) / Q) exactly (correctly rounded product and quotient): checked bit for bit
                f32 = np.float32
                det = fin & (f32(w.S - bS) == f32(w.S + bS)) & (f32(Q - bQ) == f32(Q + bQ))
                ess32 = (f32(w.S) * f32(w.S)).astype(f32) / f32(Q)
                err = np.abs(got["ess"].astype(np.float64) - ref.ess) / ref.ess
            assert (err[fin] <= tol_ess[fin]).all(), [(names[b], err[b], tol_ess[b]) for b in np.flatnonzero(fin & (err > tol_ess))[:4]]
            assert np.array_equal(got["ess"][det], ess32[det]), [(names[b], got["ess"][b], ess32[b]) for b in
                                                                 np.flatnonzero(det & (got["ess"] != ess32))[:4]]
            if K == 1:
                assert (got["ess"][fin] == 1.0).all()
            for b in np.flatnonzero(fin):
                if names[b] == "equal":
                    assert got["ess"][b] == K, (b, got["ess"][b])   # exact: every e_k is expf(0) = 1
                if names[b] == "dominant":
                    assert got["ess"][b] == 1.0, (b, got["ess"][b])   # exact: the others underflow to 0
            # evidence: rel(S) + u (S / K) + 2 ulp of log(S / K) + one rounding per add, capped at 1e-5 of max(1, |value|)
            lse_part = np.log(w.S / K)
            with np.errstate(invalid="ignore"):
                tol_ev = bS / w.S + U + S.ULP2 * np.abs(lse_part) + U * np.abs(w.lse) + U * np.abs(ref.log_evidence)
                tol_ev = np.minimum(tol_ev, CAP * np.maximum(1.0, np.abs(ref.log_evidence)))
                err = np.abs(got["log_evidence"].astype(np.float64) - ref.log_evidence)
            assert (err[fin] <= tol_ev[fin]).all(), [(names[b], err[b], tol_ev[b]) for b in np.flatnonzero(fin & (err > tol_ev))[:4]]
            # decisions: exact at ess_frac 0 and 1; elsewhere skipped inside the ESS band
            dec = ref.go.copy()
            if frac not in (0.0, 1.0):
                # an ESS fixed bit for bit above decides as the kernel compares: ess32 < fl(ess_frac K); otherwise the
                # decision is skipped inside tol_ess (+ the rounding of ess_frac K)
                dec = np.where(det, ess32 < np.float32(np.float32(frac) * np.float32(K)), dec)
                close = fin & ~det & (np.abs(ref.ess - frac * K) <= tol_ess * ref.ess + U * frac * K)
                counts["dec_skipped"] += int(close.sum())
                counts["dec_checked"] += int((fin & ~close).sum())
                dec = np.where(close, got["resampled"].astype(bool), dec)
            assert np.array_equal(got["resampled"].astype(bool), dec), np.flatnonzero(got["resampled"].astype(bool) != dec)[:8]
            if frac == 0.0:
                assert not got["resampled"].any()
            if frac == 1.0:
                assert got["resampled"][:-2].all()
            a32 = S.accumulate(lw0, lw)
            for b in range(B):
                rows = slice(b * K, (b + 1) * K)
                if not dec[b]:   # identity, a_k carried bit for bit (NaN and -inf included), evidence not banked
                    assert np.array_equal(got["src"][rows], np.arange(b * K, (b + 1) * K)), (names[b], b)
                    assert np.array_equal(got["log_w"][rows], a32[rows], equal_nan=True), (names[b], b)
                    assert got["log_z"][b] == log_z[b], (names[b], b)
                    continue
                counts["went"] += 1
                assert (got["log_w"][rows] == 0).all()
                assert abs(float(got["log_z"][b]) - (float(log_z[b]) + w.lse[b])) <= tol_ev[b]
                anc = got["src"][rows] - b * K
                assert ((anc >= 0) & (anc < K)).all() and (np.diff(anc) >= 0).all(), (names[b], anc)
                e = w.e[b]
                # a particle whose fp32 weight is 0 (-inf, or underflowed) is never chosen
                d32 = (a32[rows] - np.float32(w.m[b])).astype(np.float32)
                assert (np.exp(d32.astype(np.float64))[anc] > 1e-45).all() and np.isfinite(a32[rows][anc]).all(), (names[b], b)
                want, c, thr = S.systematic(e, u[b])
                # a threshold closer to some c_i than the band is skipped: c_i's error (<= S's), the error S carries into
                # (k + u) S / K, and the fp32 rounding of that product (exact: |thr32 - thr|; re-rounded with the device's S
                # when S is inexact).  Exact arithmetic (equal weights, one dominant particle) has a zero band: ties checked.
                t32 = _thr32(u[b], w.S[b], K)
                band = bS[b] * (1 + (np.arange(K) + u[b]) / K) + np.abs(t32 - thr) + (2 * U * thr if bS[b] > 0 else 0.0)
                near = np.abs(c[None, :] - thr[:, None]) < band[:, None]
                amb = near.any(1)
                counts["anc_skipped"] += int(amb.sum())
                if amb.any():
                    counts.setdefault("anc_skipped_in", set()).add(names[b])
                counts["anc_checked"] += int((~amb).sum())
                assert np.array_equal(anc[~amb], want[~amb]), (names[b], b, np.flatnonzero(anc != want)[:4])
                for j in np.flatnonzero(amb):   # skipped: still one of the candidates the band allows, of positive weight
                    ok = near[j] | (np.arange(K) == want[j])
                    ok[1:] |= near[j][:-1]
                    assert ok[anc[j]] and e[anc[j]] > 0, (names[b], b, j, anc[j], want[j])
    print(K, T, counts)
    assert counts["went"] > 0
    assert counts["dec_skipped"] <= 0.1 * max(1, counts["dec_checked"] + counts["dec_skipped"]), counts
    assert counts["anc_checked"] > 0 and counts["anc_skipped"] <= 0.1 * (counts["anc_checked"] + counts["anc_skipped"]), counts


def test_non_finite_lane_never_resamples(handle):
    """A lane with a NaN weight or with every weight at -inf has a non-finite ESS: for every ess_frac (1 included) it keeps the
    identity map and its weights, so the bad values stay visible; the finite lanes next to it are untouched by it."""
    lib, h = handle
    K, B, T = 4, 3, 1
    lw0 = np.zeros((B, K), np.float32)
    lw0[0, 2] = np.nan
    lw0[1, :] = -np.inf
    lw0[2] = [0.0, -1.0, -2.0, -3.0]
    lw = np.zeros((T, B * K), np.float32)
    for frac in (0.0, 0.5, 1.0):
        got = _run(lib, h, lw0.reshape(-1), lw, np.zeros(B, np.float32), T, B, K, frac, np.full(B, 0.25, np.float32),
                   np.zeros(B * K, np.int32))
        assert list(got["resampled"][:2]) == [0, 0], frac
        assert np.array_equal(got["src"][:2 * K], np.arange(2 * K))
        assert np.array_equal(got["log_w"][:2 * K], lw0.reshape(-1)[:2 * K], equal_nan=True)
        assert not np.isfinite(got["ess"][:2]).any()
        assert got["resampled"][2] == int(frac == 1.0 or frac == 0.5 and got["ess"][2] < 2.0)
