"""Float64 reference of the object layers (include/sqair_hip.h: sqair_set_layers, points 1-7; no GPU import: the CPU tests use it).

The weights, the best row's objects and the association are ``tests/estimate_ref.estimate``'s (``weights``, ``presence``, ``match``,
``agree``, ``bad``); V and O of a slot are the oracle's ``st_insert`` of its glimpse and of a glimpse of ones, times its presence, as
tests/test_hip_kernels.py::test_st_insert_loglik forms the decoder's canvas.  With ``match`` given, that table stands in for the
reference's own: the pixel values of a device run are then compared without any threshold in between.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import sqair_oracle as O
from tests import estimate_check as EC
from tests import estimate_ref as E


def slot_images(glimpse, where, presence, hw):
    """V and O of every slot, float64 [..., H, W]: ``glimpse`` [..., G, G], ``where`` [..., 4], ``presence`` [...]."""
    glimpse, where, presence = (np.asarray(x, dtype=np.float64) for x in (glimpse, where, presence))
    lead, G = presence.shape, glimpse.shape[-1]
    g = torch.as_tensor(glimpse.reshape(-1, G, G))
    wl = torch.as_tensor(where.reshape(-1, 4))
    p = presence.reshape(-1, 1, 1)
    V = O.st_insert(g, wl, hw[0], hw[1]).numpy() * p
    On = O.st_insert(torch.ones_like(g), wl, hw[0], hw[1]).numpy() * p
    return V.reshape(lead + tuple(hw)), On.reshape(lead + tuple(hw))


def owner_rule(cover, present, cover_min):
    """owner [..., H, W] of ``cover`` [..., N, H, W] (any float type: compared as it is) and ``present`` [..., N]: the first present j
    of maximal cover if that maximum is >= cover_min, else -1; a NaN never wins."""
    cover = np.asarray(cover)
    ok = np.asarray(present, dtype=bool)[..., None, None] & ~np.isnan(cover)
    c = np.where(ok, cover, -np.inf)
    j = np.argmax(c, axis=-3)                       # (the first of equal maxima)
    top = np.max(c, axis=-3)
    return np.where(top >= cover.dtype.type(cover_min), j, -1).astype(np.int64)


def layers(glimpse, where, presence, lw, K, hw, iou_min, cover_min, lw0=None, match=None):
    """The layers of every (frame t, lane b) of per-row tensors shaped [T, B*K, ...] (``glimpse`` [T, B*K, N, G, G]; ``lw``, ``lw0`` as
    estimate_ref.estimate's).  ``match`` [T, B, K, N]: taken as the association instead of the reference's own.  Returns ``match``
    (int64), ``layer``, ``cover`` [T, B, N, H, W] (float64), ``owner`` [T, B, H, W], ``present`` [T, B, N], ``bad`` [T, B] and the
    estimate it rests on (``est``)."""
    where, presence = np.asarray(where), np.asarray(presence)
    T, R, N = presence.shape
    B = R // K
    est = E.estimate(where, presence, np.zeros_like(presence), lw, K, hw, iou_min, lw0=lw0)
    m = est.match if match is None else np.asarray(match).astype(np.int64)
    present = est.presence != 0
    V, On = slot_images(glimpse, where, presence, hw)
    V, On = V.reshape((T, B, K, N) + tuple(hw)), On.reshape((T, B, K, N) + tuple(hw))
    o = SimpleNamespace(match=np.where(est.bad[:, :, None, None], -1, m), layer=np.zeros((T, B, N) + tuple(hw)),
                        cover=np.zeros((T, B, N) + tuple(hw)), present=present, bad=est.bad, est=est, support=np.zeros((T, B, N)))
    ks = np.arange(K)
    for t in range(T):
        for b in range(B):
            if est.bad[t, b]:
                o.layer[t, b] = o.cover[t, b] = np.nan
                continue
            w = est.weights[t, b]
            for j in np.flatnonzero(present[t, b]):
                a = m[t, b, :, j] >= 0
                wa = np.where(a, w, 0.0)
                s = wa.sum()
                o.support[t, b, j] = s
                sl = np.maximum(m[t, b, :, j], 0)
                with np.errstate(invalid="ignore", divide="ignore"):
                    o.layer[t, b, j] = np.tensordot(wa, V[t, b, ks, sl], 1) / s
                    o.cover[t, b, j] = np.tensordot(wa, On[t, b, ks, sl], 1) / s
    o.owner = np.where(est.bad[:, :, None, None], -1, owner_rule(o.cover, present, cover_min))
    return o


def near_decisions(est, iou_min):
    """tests/estimate_check.py's rule for a decision too close to a threshold to hold a device to: per (t, b, k, j) of a finite lane
    and a present best-row object, |best IoU - iou_min| <= 1e-5, or best and second-best IoU of different slots within 1e-5 with
    the best not clearly below iou_min.  Returns (near [T, B, K, N] bool, the number of decisions)."""
    live = (~est.bad)[:, :, None, None] & (est.presence != 0)[:, :, None, :]
    has = est.iou_best >= 0
    near_thr = has & (np.abs(est.iou_best - iou_min) <= EC.NEAR)
    near_tie = has & (est.iou_best - est.iou_second <= EC.NEAR) & (est.iou_best >= iou_min - EC.NEAR)
    live = np.broadcast_to(live, has.shape)
    return live & (near_thr | near_tie), int(live.sum())
