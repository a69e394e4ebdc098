"""Float64 reference of the lane estimate (include/sqair_hip.h: sqair_set_estimate, points 1-7; no GPU import: the CPU tests use it).

Only a_k is formed in fp32, in frame order, through ``smc_ref.accumulate``, because the header states it so; everything after it is
float64: m, e, S, ESS through ``smc_ref.weights``, the boxes through the oracle's ``to_coords`` / ``stn_to_pixel_coords``.
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import sqair_oracle as O
from tests import smc_ref as S


def boxes(where, hw):
    """(y, x, h, w) in pixels of where logits [..., 4]: stn_to_pixel_coords(to_coords(where), hw), float64."""
    co = O.to_coords(torch.as_tensor(np.asarray(where, dtype=np.float64)))
    return O.stn_to_pixel_coords(np.stack([c.numpy() for c in co], -1), hw)


def iou(p, q):
    """Axis-aligned intersection over union of boxes (y, x, h, w) [..., 4] (broadcast): overlap lengths min(y1 + h1, y2 + h2) -
    max(y1, y2) clipped at 0; 0 when the union is not positive, else exactly 1 for two boxes with the same four values."""
    p, q = np.broadcast_arrays(np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64))
    oy = np.maximum(np.minimum(p[..., 0] + p[..., 2], q[..., 0] + q[..., 2]) - np.maximum(p[..., 0], q[..., 0]), 0.0)
    ox = np.maximum(np.minimum(p[..., 1] + p[..., 3], q[..., 1] + q[..., 3]) - np.maximum(p[..., 1], q[..., 1]), 0.0)
    inter = oy * ox
    uni = p[..., 2] * p[..., 3] + q[..., 2] * q[..., 3] - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(uni > 0, inter / np.where(uni > 0, uni, 1.0), 0.0)
    return np.where((uni > 0) & (p == q).all(-1), 1.0, v)


def estimate(where, presence, obj_id, lw, K, hw, iou_min, lw0=None, what=None, canvas=None):
    """The estimate of every (frame t, lane b) of per-row tensors shaped [T, B*K, ...] (``lw`` [T, B*K] the per-frame log weights,
    ``lw0`` [B*K] the carried ones, None = zeros).  Returns the outputs of SqairLaneEstimate as float64 / int64 arrays, plus what a
    comparison against fp32 needs: ``w`` (per frame, smc_ref.weights of a_k), ``bad`` [T, B], and per (t, b, k, j) the best and
    second-best IoU of particle k's present slots with best-row object j (``iou_best``, ``iou_second``; -1 where there is none),
    ``agree`` and the matched slot ``match``."""
    where, presence, obj_id = (np.asarray(x) for x in (where, presence, obj_id))
    T, R, N = presence.shape
    B = R // K
    lw = np.asarray(lw, dtype=np.float32)
    lw0 = np.zeros(R, np.float32) if lw0 is None else np.asarray(lw0, dtype=np.float32)
    nan = np.nan
    o = SimpleNamespace(
        weights=np.zeros((T, B, K)), ess=np.zeros((T, B)), best_row=np.zeros((T, B), np.int64), count_prob=np.zeros((T, B, N + 1)),
        expected_count=np.zeros((T, B)), map_count=np.zeros((T, B), np.int64), presence=np.zeros((T, B, N), presence.dtype),
        obj_id=np.zeros((T, B, N), obj_id.dtype), where=np.zeros((T, B, N, 4), where.dtype), box=np.zeros((T, B, N, 4)),
        support=np.zeros((T, B, N)), box_mean=np.zeros((T, B, N, 4)), w=[], bad=np.zeros((T, B), bool),
        iou_best=np.full((T, B, K, N), -1.0), iou_second=np.full((T, B, K, N), -1.0), agree=np.zeros((T, B, K, N), bool),
        match=np.full((T, B, K, N), -1, np.int64), what=None, mean_canvas=None, a=np.zeros((T, R), np.float32))
    if what is not None:
        what = np.asarray(what)
        o.what = np.zeros((T, B, N) + what.shape[3:], what.dtype)
    if canvas is not None:
        canvas = np.asarray(canvas, dtype=np.float64)
        o.mean_canvas = np.zeros((T, B) + canvas.shape[2:])
    box_all = boxes(where, hw).reshape(T, B, K, N, 4)
    pres_all = (presence != 0).reshape(T, B, K, N)
    for t in range(T):
        a = S.accumulate(lw0, lw[:t + 1])
        o.a[t] = a
        w = S.weights(a, K)
        o.w.append(w)
        bad = ~np.isfinite(w.S)
        o.bad[t] = bad
        with np.errstate(invalid="ignore", divide="ignore"):
            wk = w.e / w.S[:, None]
            o.ess[t] = w.ess
        wk[bad] = nan
        o.weights[t] = wk
        a2 = a.reshape(B, K)
        for b in range(B):
            pk, bx = pres_all[t, b], box_all[t, b]             # [K, N], [K, N, 4]
            if bad[b]:
                o.best_row[t, b] = o.map_count[t, b] = -1
                o.count_prob[t, b] = o.expected_count[t, b] = nan
                o.support[t, b] = o.box_mean[t, b] = nan
                if o.mean_canvas is not None:
                    o.mean_canvas[t, b] = nan
                continue
            kb = int(np.argmax(a2[b]))                          # the first k of maximal a_k (fp32: an exact compare)
            r = b * K + kb
            o.best_row[t, b] = r
            n = pk.sum(1)
            o.count_prob[t, b] = (wk[b][None, :] * (n[None, :] == np.arange(N + 1)[:, None])).sum(1)
            o.expected_count[t, b] = (wk[b] * n).sum()
            o.map_count[t, b] = int(np.argmax(o.count_prob[t, b]))   # the first c of maximal probability
            pj = pk[kb]
            o.presence[t, b] = np.where(pj, presence[t, r], 0)
            o.obj_id[t, b] = np.where(pj, obj_id[t, r], 0)
            o.where[t, b] = np.where(pj[:, None], where[t, r], 0)
            o.box[t, b] = np.where(pj[:, None], bx[kb], 0.0)
            if o.what is not None:
                o.what[t, b] = np.where(pj.reshape((N,) + (1,) * (what.ndim - 3)), what[t, r], 0)
            # v[k, j, m] = IoU(best-row box j, box of (k, m)), -1 where slot m of row k is absent
            v = np.where(pk[:, None, :], iou(bx[kb][None, :, None, :], bx[:, None, :, :]), -1.0)
            ms = np.argmax(v, -1)                               # the first slot of maximal IoU
            top = np.sort(v, -1)
            best = top[..., -1]
            o.iou_best[t, b] = np.where(pj[None, :], best, -1.0)
            if N > 1:
                o.iou_second[t, b] = np.where(pj[None, :], top[..., -2], -1.0)
            agree = (best >= iou_min) & pj[None, :]
            o.agree[t, b] = agree
            o.match[t, b] = np.where(agree, ms, -1)
            for j in np.flatnonzero(pj):
                wa = np.where(agree[:, j], wk[b], 0.0)
                sup = wa.sum()
                o.support[t, b, j] = sup
                with np.errstate(invalid="ignore", divide="ignore"):
                    o.box_mean[t, b, j] = (wa[:, None] * bx[np.arange(K), ms[:, j]]).sum(0) / sup
            if o.mean_canvas is not None:
                o.mean_canvas[t, b] = np.tensordot(wk[b], canvas[t, b * K:(b + 1) * K], 1)
    return o
