"""Float64 reference of the lane forecast (include/sqair_hip.h: sqair_forecast_fan, points 1-7; no GPU import: the CPU tests use it),
and the generator of synthetic rollouts the CPU and GPU tests share.

Only the log weights are taken in fp32 (they are the caller's fp32 words; an exact compare picks the best row); everything after is
float64: m, e, S through ``smc_ref.weights``, the boxes and the IoU through ``estimate_ref``.
"""
from types import SimpleNamespace

import numpy as np

from tests import estimate_ref as E
from tests import smc_ref as S


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def lane_forecast(start_where, start_presence, start_obj_id, where, presence, obj_id, log_w, K, S_fan, hw, iou_min):
    """The lane forecast of start rows [R, N, .] (R = B*K) and their rollouts [F, R*S, N, .], rollout s of row r at r*S + s;
    ``log_w`` [R] fp32 or None (uniform).  Returns the outputs of SqairForecastLane as float64 / int64 arrays (copied words keep their
    dtype) plus what a comparison against fp32 needs: ``w`` (smc_ref.weights), ``bad`` [B], per (b, k, j) ``iou_best`` /
    ``iou_second`` of particle k's present start slots with object j (-1: none), ``agree``, ``match`` (the start slot), and per
    (f, b, q, j) ``hit`` (rollout q contributes) and ``slot`` (where it found the id)."""
    start_where, start_presence, start_obj_id, where, presence, obj_id = (
        np.asarray(x) for x in (start_where, start_presence, start_obj_id, where, presence, obj_id))
    R, N = start_presence.shape
    F = presence.shape[0]
    B, KS = R // K, K * S_fan
    a = np.zeros(R, np.float32) if log_w is None else np.asarray(log_w, dtype=np.float32)
    w = S.weights(a, K)
    bad = ~np.isfinite(w.S)
    with np.errstate(invalid="ignore", divide="ignore"):
        wk = w.e / w.S[:, None]
    wk[bad] = np.nan
    nan = np.nan
    o = SimpleNamespace(
        w=w, bad=bad, weights=wk, best_row=np.zeros(B, np.int64), start_where=start_where.copy(), start_presence=start_presence.copy(),
        start_obj_id=start_obj_id.copy(), obj_id=np.zeros((B, N), start_obj_id.dtype), presence=np.zeros((B, N), start_presence.dtype),
        box0=np.zeros((B, N, 4)), support=np.zeros((B, N)), alive=np.zeros((F, B, N)), box_mean=np.zeros((F, B, N, 4)),
        box_std=np.zeros((F, B, N, 4)), count_prob=np.zeros((F, B, N + 1)), iou_best=np.full((B, K, N), -1.0),
        iou_second=np.full((B, K, N), -1.0), agree=np.zeros((B, K, N), bool), match=np.full((B, K, N), -1, np.int64),
        hit=np.zeros((F, B, KS, N), bool), slot=np.full((F, B, KS, N), -1, np.int64))
    box_s = E.boxes(start_where, hw).reshape(B, K, N, 4)
    pres_s = (start_presence != 0).reshape(B, K, N)
    id_s = _bits(start_obj_id).reshape(B, K, N)
    box_r = E.boxes(where, hw).reshape(F, B, KS, N, 4)
    pres_r = (presence != 0).reshape(F, B, KS, N)
    id_r = _bits(obj_id).reshape(F, B, KS, N)
    a2 = a.reshape(B, K)
    kq = np.arange(KS) // S_fan                                   # the particle of rollout q
    for b in range(B):
        if bad[b]:
            o.best_row[b] = -1
            o.support[b] = o.alive[:, b] = o.box_mean[:, b] = o.box_std[:, b] = o.count_prob[:, b] = nan
            continue
        wq = wk[b][kq] / S_fan
        kb = int(np.argmax(a2[b]))                                # the first k of maximal log weight (fp32: an exact compare)
        r = b * K + kb
        o.best_row[b] = r
        pk, bx = pres_s[b], box_s[b]
        pj = pk[kb]
        o.presence[b] = np.where(pj, start_presence[r], 0)
        o.obj_id[b] = np.where(pj, start_obj_id[r], 0)
        o.box0[b] = np.where(pj[:, None], bx[kb], 0.0)
        for f in range(F):
            n = pres_r[f, b].sum(1)
            o.count_prob[f, b] = (wq[None, :] * (n[None, :] == np.arange(N + 1)[:, None])).sum(1)
        # v[k, j, m] = IoU(best-row box j, box of start slot (k, m)), -1 where slot m of row k is absent
        v = np.where(pk[:, None, :], E.iou(bx[kb][None, :, None, :], bx[:, None, :, :]), -1.0)
        ms = np.argmax(v, -1)                                     # the first slot of maximal IoU
        top = np.sort(v, -1)
        best = top[..., -1]
        o.iou_best[b] = np.where(pj[None, :], best, -1.0)
        if N > 1:
            o.iou_second[b] = np.where(pj[None, :], top[..., -2], -1.0)
        agree = (best >= iou_min) & pj[None, :]
        o.agree[b] = agree
        o.match[b] = np.where(agree, ms, -1)
        fid = id_s[b][np.arange(K)[:, None], ms]                  # [K, N] the id word followed for object j in particle k's rollouts
        for j in np.flatnonzero(pj):
            o.support[b, j] = np.where(agree[:, j], wk[b], 0.0).sum()
            for f in range(F):
                same = pres_r[f, b] & (id_r[f, b] == fid[kq, j][:, None]) & agree[kq, j][:, None]    # [KS, N]
                hit = same.any(1)
                slot = np.argmax(same, 1)                         # the first such slot
                o.hit[f, b, :, j] = hit
                o.slot[f, b, :, j] = np.where(hit, slot, -1)
                wa = np.where(hit, wq, 0.0)
                al = wa.sum()
                o.alive[f, b, j] = al
                x = box_r[f, b][np.arange(KS), slot]              # [KS, 4]
                with np.errstate(invalid="ignore", divide="ignore"):
                    mean = (wa[:, None] * x).sum(0) / al
                    o.box_mean[f, b, j] = mean
                    o.box_std[f, b, j] = np.sqrt((wa[:, None] * (x - mean) ** 2).sum(0) / al)
    return o


# ---- synthetic rollouts ---------------------------------------------------------------------------------------------------------
PATTERNS = ("random", "equal", "dominant", "spread", "neg_inf")
SIGMAS = (0.02, 0.15, 0.5)
TINY_SCALE_LOGIT = -1.0e4   # a scale logit at the floor of to_coords (sigmoid kept >= 1e-4): the smallest box the formula gives --
                            # sq_box_of_where cannot give an area of exactly zero, this is the degenerate box it can give


def make_rollouts(K, S_fan, F, N, per_cell, rng, big_boxes=False):
    """Start rows and rollouts of B = per_cell * 15 + 6 lanes: SimpleNamespace(B, start_where [R, N, 4], start_presence,
    start_obj_id [R, N], where [F, R*S, N, 4], presence, obj_id [F, R*S, N], log_w [R], names).

    A lane's particles are jittered copies of a base scene (sigma per lane: all associate / the threshold cuts through them / few do)
    with random presence, holes included, and ids that are distinct within a row and differ between rows.  In a rollout every
    start object has a death frame (possibly never): it stays dead, the survivors random-walk, and each frame is compacted
    present-first in a stable order with id -1 behind them -- so ids move between slots.  Special lanes, after the grid of weight
    patterns: ``twin`` (best-row objects 0 and 1 share a box and odd particles hold only one of them: two objects follow one id),
    ``tiny`` (object 0 has the degenerate box of TINY_SCALE_LOGIT), ``fresh`` (the best row is a fresh one: nothing present, ids -1),
    then ``nan``, ``pos_inf`` and ``all_neg_inf`` (the three kinds of non-finite lane)."""
    cells = [(p, s) for p in PATTERNS for s in SIGMAS]
    special = ["twin", "tiny", "fresh", "nan", "pos_inf", "all_neg_inf"]
    B = per_cell * len(cells) + len(special)
    sig = np.array([s for _, s in cells for _ in range(per_cell)] + [0.15] * len(special))
    names = [p for p, _ in cells for _ in range(per_cell)] + special
    R, KS = B * K, K * S_fan
    base = rng.standard_normal((B, 1, N, 4))
    base[..., :2] = base[..., :2] * 0.7 + (3.0 if big_boxes else -1.0)
    i_twin, i_tiny, i_fresh = (names.index(n) for n in ("twin", "tiny", "fresh"))
    sig[i_twin] = 0.02                                            # (every particle associates with the twins)
    if N > 1:
        base[i_twin, 0, 1] = base[i_twin, 0, 0]
    base[i_tiny, 0, 0, :2] = TINY_SCALE_LOGIT
    sw = base + sig[:, None, None, None] * rng.standard_normal((B, K, N, 4))
    sw[i_tiny, :, 0, :2] = TINY_SCALE_LOGIT
    n_obj = rng.integers(0, N + 1, size=B)
    n_obj[0::7] = 0
    n_obj[1::7] = N
    n_obj[[i_twin, i_tiny]] = N
    base_p = np.arange(N)[None, :] < n_obj[:, None]
    flip = rng.uniform(size=(B, K, N)) < 0.15
    flip[0::7] = False
    flip[1::7] = False
    flip[[i_twin, i_tiny]] = False
    sp = base_p[:, None, :] ^ flip
    if N > 1:
        sp[i_twin, 1::2, 1] = False                               # odd particles hold only object 0 of the twins
    sid = np.argsort(rng.uniform(size=(B, K, 50)), -1)[..., :N].astype(np.float64)   # distinct within a row
    lw = np.zeros((B, K), np.float32)
    for b, name in enumerate(names):
        if name in ("random", "twin", "tiny"):
            lw[b] = rng.standard_normal(K) * 2
        elif name == "equal":
            lw[b] = rng.standard_normal() * 5
        elif name == "dominant":
            lw[b] = -np.inf if b % 2 == 0 else -200.0
            lw[b, rng.integers(0, K)] = 0.0
        elif name == "spread":
            lw[b] = -rng.uniform(size=K) * rng.uniform(80, 110)
        elif name == "neg_inf":
            lw[b] = rng.standard_normal(K)
            dead = rng.uniform(size=K) < 0.4
            dead[rng.integers(0, K)] = False
            lw[b] = np.where(dead, -np.inf, lw[b])
    lw[i_twin, 0] = 5.0                                           # (an even particle is the best row: it holds both twins)
    lw[i_fresh] = rng.standard_normal(K)
    k_fresh = int(np.argmax(lw[i_fresh]))
    sp[i_fresh, k_fresh] = False
    sid[i_fresh, k_fresh] = -1.0
    sw[i_fresh, k_fresh] = 0.0
    lw[names.index("nan"), K // 2] = np.nan
    lw[names.index("pos_inf"), K - 1] = np.inf
    lw[names.index("all_neg_inf")] = -np.inf
    sid = np.where(sp, sid, -1.0)                                 # (an absent slot carries id -1, as a pass leaves it)
    # rollouts
    death = rng.integers(0, F + 3, size=(B, K, S_fan, N))         # object dies AT frame death (>= F: never within the horizon)
    walk = np.cumsum(0.1 * rng.standard_normal((F, B, K, S_fan, N, 4)), 0)
    where = np.zeros((F, B, K, S_fan, N, 4))
    pres = np.zeros((F, B, K, S_fan, N), bool)
    ids = np.full((F, B, K, S_fan, N), -1.0)
    for f in range(F):
        live = sp[:, :, None, :] & (death > f)                    # [B, K, S, N] by start slot
        order = np.argsort(~live, -1, kind="stable")              # present first, stable
        src_w = sw[:, :, None, :, :] + walk[f]
        src_w[..., :2] = np.where((sw[:, :, None, :, :2] == TINY_SCALE_LOGIT), TINY_SCALE_LOGIT, src_w[..., :2])
        pres[f] = np.take_along_axis(live, order, -1)
        ids[f] = np.where(pres[f], np.take_along_axis(np.broadcast_to(sid[:, :, None, :], live.shape), order, -1), -1.0)
        where[f] = np.take_along_axis(src_w, order[..., None], -2)
    f32 = np.float32
    return SimpleNamespace(B=B, names=names, start_where=sw.reshape(R, N, 4).astype(f32), start_presence=sp.reshape(R, N).astype(f32),
                           start_obj_id=sid.reshape(R, N).astype(f32), where=where.reshape(F, R * S_fan, N, 4).astype(f32),
                           presence=pres.reshape(F, R * S_fan, N).astype(f32), obj_id=ids.reshape(F, R * S_fan, N).astype(f32),
                           log_w=lw.reshape(R))


def near_threshold(ref, iou_min, near=1e-5):
    """(decisions, skipped): the association decisions of ``ref`` (one per present best-row object and particle) and those among them
    a comparison against fp32 skips: the best IoU within ``near`` of iou_min, or the two best within ``near`` of each other with the
    best not clearly below iou_min (tests/estimate_check.py's rule)."""
    pj = (ref.presence != 0)[:, None, :] & ~ref.bad[:, None, None]
    best, second = ref.iou_best, ref.iou_second
    has = pj & (best >= 0)
    skip = has & ((np.abs(best - iou_min) <= near) | ((best - second <= near) & (best >= iou_min - near)))
    K = best.shape[1]
    return int(pj.any(1).sum()) * K, skip


# ---- the cases of tests/test_forecast_lane_kernel.py (here, so that the CPU test can hold their inputs against the 1 % cap) ----------
# (K, S, F, N, wide, hw, iou_min): one wave, a wave boundary, every thread of the workgroup and four rollouts per thread; N = 14 is
# the most a handle takes (tests/test_estimate_kernel.py)
CASES = [(K, S, F, 4, False, (50, 50), 0.5) for K, S in ((1, 1), (1, 8), (2, 3), (5, 4), (64, 1), (65, 3), (256, 4)) for F in (1, 3)]
CASES.append((5, 4, 3, 14, True, (50, 50), 0.3))
CASES.append((65, 3, 3, 4, False, (12, 9), 0.7))


def case_id(c):
    return "K{}_S{}_F{}_N{}_{}x{}{}".format(c[0], c[1], c[2], c[3], c[5][0], c[5][1], "_wide" if c[4] else "")


def case_inputs(c):
    K, S_fan, F, N, wide, hw, iou_min = c
    rng = np.random.default_rng(100000 * K + 1000 * S_fan + 10 * F + N)
    return make_rollouts(K, S_fan, F, N, 1 if K * S_fan > 200 else 3, rng, big_boxes=hw != (50, 50))
