"""Float64 references for the device random numbers and the SMC resampler (no GPU import: the CPU tests use it too).

- ``philox4x32_10``: a NumPy uint64 restatement of the device generator (sqair_amd/csrc/sqair_common.h), vectorised.
- ``fill_noise``: what ``sqair_fill_noise`` (k_fill_noise, sqair_train.hip) writes, element by element.
- ``smc_uniform``: the uniform ``k_smc_resample`` draws for a lane when the caller gives none.
- ``resample``: the systematic resampler of include/sqair_hip.h (sqair_set_smc) in float64.  Only a_k is formed in fp32 in
  frame order, because the header states it so; m, e, S, ESS, the evidence, the thresholds and the search are float64.
- ``ParticleFilter``: the fp64 oracle run as a particle filter with its state carried from step to step, its rows gathered
  through a source map the caller gives (so that a device run and this one stay on the same trajectory).
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import sqair_oracle as O

MASK = np.uint64(0xFFFFFFFF)
PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
PHILOX_W = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))
SMC_TAG = 0x534D4352          # counter word 1 of the SMC uniforms ("SMCR")
U24 = 1.0 / 16777216.0        # 2^-24
FP32_EPS = 2.0 ** -24         # unit roundoff of fp32 (round to nearest)
ULP2 = 2.0 ** -22             # two ulps at 1: the accuracy assumed of the device's expf / logf


def philox4x32_10(ctr, key):
    """ctr = (c0, c1, c2, c3), key = (k0, k1): integers or arrays (broadcast), 32-bit words.  Returns four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & MASK for x in ctr]
    k0, k1 = (np.asarray(x, dtype=np.uint64) & MASK for x in key)
    for _ in range(10):
        p0, p1 = PHILOX_M[0] * c[0], PHILOX_M[1] * c[2]   # (32 x 32 -> 64 bits: exact in uint64)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & MASK]
        k0, k1 = (k0 + PHILOX_W[0]) & MASK, (k1 + PHILOX_W[1]) & MASK
    return [x.astype(np.uint32) for x in c]


def _split64(v):
    v = np.asarray(v, dtype=np.uint64)
    return v & MASK, v >> np.uint64(32)


def fill_noise(T, B, K, N, n_what, seed, step, global_B=None, b0=0):
    """sqair_fill_noise(noise, T, B, global_B, b0, seed, step) for a configuration (K, N, n_what): [T, B*K, 2, N, 4+n_what+1]
    float64.  Element e of the local buffer is global element g = t * (per frame, global batch) + b0 * K * per_row + (e within
    its frame); counter (g lo, g hi, step lo, step hi), key (seed lo, seed hi).  The last entry of a record is u = (w2 >> 8) 2^-24
    (exactly the device's fp32 value); the others are Box-Muller eps = sqrt(-2 log u1) cos(2 pi' u2), u1 = ((w0 >> 8) + 1) 2^-24,
    u2 = (w1 >> 8) 2^-24, with 2 pi' the device's fp32 constant and its fp32 product with u2 (the rest in float64)."""
    global_B = B if global_B is None else global_B
    nzw = 4 + n_what + 1
    per_row = 2 * N * nzw
    pfl, pfg = B * K * per_row, global_B * K * per_row
    e = np.arange(T * pfl, dtype=np.uint64)
    t = e // np.uint64(pfl)
    g = t * np.uint64(pfg) + np.uint64(b0 * K * per_row) + (e - t * np.uint64(pfl))
    glo, ghi = _split64(g)
    slo, shi = _split64(step)
    klo, khi = _split64(seed)
    w = philox4x32_10((glo, ghi, slo, shi), (klo, khi))
    u = (w[2] >> np.uint32(8)).astype(np.float64) * U24
    u1 = ((w[0] >> np.uint32(8)).astype(np.float64) + 1.0) * U24
    u2 = (w[1] >> np.uint32(8)).astype(np.float32) * np.float32(U24)
    arg = (np.float32(6.28318530717958647692) * u2).astype(np.float64)
    eps = np.sqrt(-2.0 * np.log(u1)) * np.cos(arg)
    is_u = (g % np.uint64(nzw)) == np.uint64(nzw - 1)
    return np.where(is_u, u, eps).reshape(T, B * K, 2, N, nzw)


def smc_uniform(b, counter, seed):
    """The lane uniform of k_smc_resample without caller uniforms: Philox counter (b, SMC_TAG, counter, 0), key (seed lo,
    seed hi), word 0 -> (w0 >> 8) 2^-24.  ``counter`` = the frame counter of row b*K after the pass."""
    b = np.asarray(b, dtype=np.uint64)
    klo, khi = _split64(seed)
    w = philox4x32_10((b, np.uint64(SMC_TAG), np.asarray(counter, dtype=np.int64).astype(np.uint64) & MASK, np.uint64(0)),
                      (klo, khi))
    return ((w[0] >> np.uint32(8)).astype(np.float64) * U24).astype(np.float32)


def accumulate(lw0, lw):
    """a_k = the carried log weight plus this pass's per-frame log weights, in frame order, in fp32 (the header's contract)."""
    a = np.asarray(lw0, dtype=np.float32).copy()
    for t in range(lw.shape[0]):
        a = (a + np.asarray(lw[t], dtype=np.float32)).astype(np.float32)
    return a


def weights(a, K):
    """float64 m, e, S, ESS and log(S / K) + m of a [B*K] (any dtype) per lane; non-finite lanes give a non-finite ESS."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, K)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = a.max(1)
        e = np.exp(a - m[:, None])
        S = e.sum(1)
        ess = S * S / (e * e).sum(1)
        lse = m + np.log(S / K)
    return SimpleNamespace(a=a, m=m, e=e, S=S, ess=ess, lse=lse)


def systematic(e, u):
    """Ancestors (within the lane) of the systematic resampler: output j = the smallest i with c_i > (j + u) S / K, c the
    inclusive prefix of e; if none, the first i with c_i = S (the last particle of positive weight).  float64."""
    K = e.shape[0]
    c = np.cumsum(e)
    thr = (np.arange(K) + np.float64(u)) * c[-1] / K
    anc = np.searchsorted(c, thr, side="right")
    last = int(np.searchsorted(c, c[-1], side="left"))
    return np.where(anc >= K, last, anc), c, thr


def rounding_band(w, K):
    """Per lane, an fp32 bound (first order) on |S_device - S|, the absolute error of the device's fixed-order sum of
    e_k = expf(fl(a_k - m)): each e_k carries u |a_k - m| (the subtraction) + 2 ulp (expf), each addition of the prefix u |c_i|
    unless it is exact in fp32 (then 0: integer and equal-weight sums are exact)."""
    a, m, e = w.a, w.m, w.e
    with np.errstate(invalid="ignore"):
        d = np.abs(a - m[:, None])
        exact_e = (d == 0) | (e == 0)   # expf(0) = 1 and expf(-inf) = 0 exactly
        err_e = np.where(exact_e, 0.0, e * (FP32_EPS * d + ULP2))
        e32 = e.astype(np.float32)
        c32 = np.cumsum(e32.astype(np.float64), axis=1)   # (a sum of two fp32 values is exact in float64)
        prev = np.concatenate([np.zeros((e.shape[0], 1)), c32[:, :-1]], 1)
        inexact = (prev.astype(np.float32) + e32).astype(np.float64) != prev + e32
        err_sum = FP32_EPS * np.where(inexact, np.abs(c32), 0.0)
    return np.nan_to_num(err_e.sum(1) + err_sum.sum(1), nan=np.inf)


def resample(lw0, lw, log_z, u, K, ess_frac):
    """The whole kernel in float64 (a_k in fp32): ESS, evidence, decision, source map and the carried weights, per lane.
    lw0 [B*K] carried log weights, lw [T, B*K] this pass's, log_z [B], u [B] the lanes' uniforms."""
    a = accumulate(lw0, lw)
    B = a.shape[0] // K
    w = weights(a, K)
    log_z = np.asarray(log_z, dtype=np.float64)
    finite = np.isfinite(w.ess)
    go = finite & ((ess_frac == 1.0) | (w.ess < ess_frac * K))
    src = np.arange(B * K)
    anc = np.tile(np.arange(K), (B, 1))
    for b in np.flatnonzero(go):
        anc[b] = systematic(w.e[b], u[b])[0]
        src[b * K:(b + 1) * K] = b * K + anc[b]
    log_w = np.where(np.repeat(go, K), np.float32(0.0), a).astype(np.float32)
    return SimpleNamespace(a=a, w=w, ess=w.ess, log_evidence=log_z + w.lse, go=go, src=src, anc=anc, log_w=log_w,
                           log_z=np.where(go, log_z + w.lse, log_z))


class ParticleFilter(object):
    """The fp64 oracle as a particle filter over B lanes of K particles.  ``propose`` runs the oracle on a step's frames from the
    carried state without committing anything (the caller may reject the noise); ``commit`` takes the result, adds the step's
    per-frame log weights to the carried ones and returns ESS and the evidence per lane; ``advance`` gathers the state through a
    source map given by the caller (-1: a fresh row) and banks or carries the weights of each lane as the caller's
    ``resampled`` says; ``reset`` zeroes a lane's weights and evidence (its rows start fresh through the next map)."""

    def __init__(self, P, F, hw, B):
        self.orc = O.SqairOracle(P, O.make_cfg(F, hw), torch.float64)
        self.B, self.K = int(B), int(F.k_particles)
        self.R = self.B * self.K
        self.state = self.orc.initial_state(self.R)
        self.log_w = np.zeros(self.R)      # float64: log weights since the lane's last resampling
        self.log_z = np.zeros(self.B)      # float64: evidence banked at resamplings
        self.a = None

    def propose(self, frames, noise):
        tiled = O.tile_input_for_iwae(torch.as_tensor(np.asarray(frames), dtype=torch.float64), self.K)
        with torch.no_grad():
            return self.orc.sequence(tiled, torch.as_tensor(np.asarray(noise), dtype=torch.float64), state=self.state,
                                     return_state=True)

    def commit(self, proposal):
        out, self.state = proposal
        lw = out["log_weights_per_timestep"].numpy()
        self.a = self.log_w + lw.sum(0)
        w = weights(self.a, self.K)
        return out, SimpleNamespace(w=w, ess=w.ess, log_evidence=self.log_z + w.lse)

    def advance(self, src, resampled):
        src = np.asarray(src, dtype=np.int64)
        go = np.asarray(resampled).astype(bool)
        lse = weights(self.a, self.K).lse
        self.state = self.orc.gather_state(self.state, src)
        self.log_z = np.where(go, self.log_z + lse, self.log_z)
        self.log_w = np.where(np.repeat(go, self.K), 0.0, self.a)   # (a lane that did not resample keeps the identity map)

    def reset(self, lanes):
        for j in lanes:
            self.log_w[j * self.K:(j + 1) * self.K] = 0.0
            self.log_z[j] = 0.0
