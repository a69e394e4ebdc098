"""Float64 reference of the lane tracks (include/sqair_hip.h: sqair_history_trace_lane, points 1-7; no GPU import: the CPU tests use
it), and the generator of synthetic traced paths the CPU and GPU tests share.

The lane tracks are the lane forecast run backwards in time: the newest traced frame F - 1 stands where the forecast's start rows
stand, the older frames where its rollouts stand (S = 1), and a row that is invalid at a frame holds nothing there.  So points 1-4 are
``forecast_lane_ref.lane_forecast`` on the masked rows in reversed frame order -- the float64 code the lane forecast is held against
-- and what the tracks add is computed here: the unnormalised ``count_prob`` and ``valid_mass`` (point 5: an invalid row counts
nowhere, not even as "zero objects") and ``first_frame`` (point 6).
"""
from types import SimpleNamespace

import numpy as np

from tests import forecast_lane_ref as FL

PER_FRAME = ("alive", "box_mean", "box_std", "hit", "slot")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def masked(presence, valid):
    """The presence words of the traced rows with every slot of an invalid (frame, row) absent."""
    presence = np.asarray(presence)
    return np.where(np.asarray(valid)[..., None] != 0, presence, np.zeros((), presence.dtype))


def lane_tracks(where, presence, obj_id, valid, log_w, K, hw, iou_min):
    """The lane tracks of traced rows [F, R, N, .] (R = B*K, frames oldest -> newest) with their mask ``valid`` [F, R]; ``log_w`` [R]
    fp32 or None (uniform).  Returns the outputs of SqairTraceLane as float64 / int64 arrays (copied words keep their dtype), frames
    oldest -> newest, plus the reference's own bookkeeping as ``lane_forecast`` returns it (``w``, ``bad``, ``iou_best``,
    ``iou_second``, ``agree``, ``match``, and per (f, b, k, j) ``hit`` and ``slot``), and ``fwd``: that same result in the forecast's
    frame order (frame 0 = F - 2, ...; F - 1 is its start), what tests/forecast_lane_check.py compares against."""
    where, presence, obj_id, valid = (np.asarray(x) for x in (where, presence, obj_id, valid))
    F, R, N = presence.shape
    B = R // K
    pm = masked(presence, valid)
    # points 1-4: the forecast's reference, start = frame F - 1, "rollout" frame i = traced frame F - 1 - i (i = 0 is the start frame
    # itself: there alive is the support)
    fwd = FL.lane_forecast(where[F - 1], pm[F - 1], obj_id[F - 1], where[::-1], pm[::-1], obj_id[::-1], log_w, K, 1, hw, iou_min)
    o = SimpleNamespace(**{k: v for k, v in vars(fwd).items() if not k.startswith("start_")})
    for name in PER_FRAME:
        setattr(o, name, getattr(fwd, name)[::-1].copy())
    o.fwd = fwd
    # point 5: counts over the valid rows, unnormalised
    wk = o.weights
    ok = (valid != 0).reshape(F, B, K)
    n = (pm != 0).reshape(F, B, K, N).sum(-1)
    o.count_prob = np.zeros((F, B, N + 1))
    o.valid_mass = np.zeros((F, B))
    o.first_frame = np.full((B, N), -1, np.int64)
    ids = _bits(obj_id).reshape(F, B, K, N)
    pres = (pm != 0).reshape(F, B, K, N)
    for b in range(B):
        if o.bad[b]:
            o.count_prob[:, b] = o.valid_mass[:, b] = np.nan
            continue
        for f in range(F):
            wv = np.where(ok[f, b], wk[b], 0.0)
            o.valid_mass[f, b] = wv.sum()
            o.count_prob[f, b] = (wv[None, :] * (n[f, b][None, :] == np.arange(N + 1)[:, None])).sum(1)
        # point 6: the best row's own path, back from F - 1 while it is valid and holds the id present
        kb = int(o.best_row[b]) - b * K
        for j in np.flatnonzero(o.presence[b] != 0):
            idw = ids[F - 1, b, kb, j]
            for f in range(F - 1, -1, -1):
                if not ok[f, b, kb] or not (pres[f, b, kb] & (ids[f, b, kb] == idw)).any():
                    break
                o.first_frame[b, j] = f
    return o


# ---- synthetic traced paths -------------------------------------------------------------------------------------------------------
def make_paths(case):
    """Traced rows of B lanes for a case (K, F, N, wide, hw, iou_min): SimpleNamespace(B, names, where [F, R, N, 4], presence,
    obj_id [F, R, N], valid [F, R] int32, log_w [R], coalesced [B] bool), frames oldest -> newest.

    ``forecast_lane_ref.make_rollouts`` run backwards: its start rows are the newest frame, its rollout frame i the traced frame
    F - 2 - i -- so an object that dies in a rollout is an object BORN inside the window (no particle holds it at older frames: alive 0,
    NaN statistics), compaction moves ids between slots, and the special lanes are its own: twins, a degenerate box, a best row whose
    newest frame is empty, the three non-finite lanes.  Added here, what only a genealogy has:
    * coalescence: in every second ordinary lane each particle k has a donor d[k] <= k whose whole path it shares -- the same
      presence and ids in every frame -- with its own boxes only in the frames newer than a depth c; older than that the rows are
      word-for-word copies (the common ancestor);
    * paths that end fresh: a row is valid only in its newest v frames (v = 0: an empty path, the -1 of a source map; donors pass
      their v on), and older than that its words are zero, as the trace's gather leaves them -- except in every third lane, where
      they keep what the generator put there, so that the mask itself is what excludes them."""
    K, F, N, wide, hw, iou_min = case
    rng = np.random.default_rng(1000000 + 100000 * K + 1000 * F + 10 * N + (0 if hw == (50, 50) else 7))
    per_cell = 1 if K > 200 else 3
    g = FL.make_rollouts(K, 1, max(F - 1, 1), N, per_cell, rng, big_boxes=hw != (50, 50))
    B, R = g.B, g.B * K
    i_twin = g.names.index("twin")                                 # (an even particle of the twins' lane is the best row, at any K)
    g.log_w[i_twin * K] = g.log_w[i_twin * K:(i_twin + 1) * K].max() + np.float32(1.0)
    # newest -> oldest: i = 0 the start rows, i = 1.. the rollouts
    where = np.concatenate([g.start_where[None], g.where], 0)[:F].reshape(F, B, K, N, 4).copy()
    pres = np.concatenate([g.start_presence[None], g.presence], 0)[:F].reshape(F, B, K, N).copy()
    ids = np.concatenate([g.start_obj_id[None], g.obj_id], 0)[:F].reshape(F, B, K, N).copy()
    ordinary = np.array([n not in ("twin", "tiny", "fresh", "nan", "pos_inf", "all_neg_inf") for n in g.names])
    coalesced = np.zeros(B, bool)
    v = np.full((B, K), F)
    ends = rng.uniform(size=(B, K)) < 0.25
    v[ends] = rng.integers(0, F + 1, size=int(ends.sum()))
    v[~ordinary] = F
    for b in np.flatnonzero(ordinary)[::2]:
        if K == 1 or F == 1:
            break
        coalesced[b] = True
        d = np.minimum(np.arange(K), rng.integers(0, K, size=K))
        d = d[d]                                                   # (a donor of depth one is enough; d[d] <= d keeps d[k] <= k)
        c = int(rng.integers(1, F))
        own = where[:c, b].copy()
        jitter = where[:c, b] - where[:c, b][:, d]                 # k's own offset from its donor in the newer frames
        where[:, b], pres[:, b], ids[:, b] = where[:, b][:, d], pres[:, b][:, d], ids[:, b][:, d]
        where[:c, b] += 0.1 * jitter.astype(np.float32)
        same = d == np.arange(K)
        where[:c, b][:, same] = own[:, same]
        v[b] = v[b][d]
    valid = (np.arange(F)[:, None, None] < v[None]).astype(np.int32)          # [F, B, K] by i
    zero = (np.arange(B) % 3 != 2)[None, :, None] & (valid == 0)
    where[zero], pres[zero], ids[zero] = 0.0, 0.0, 0.0
    flip = lambda x: np.ascontiguousarray(x[::-1])
    return SimpleNamespace(B=B, names=g.names, where=flip(where).reshape(F, R, N, 4), presence=flip(pres).reshape(F, R, N),
                           obj_id=flip(ids).reshape(F, R, N), valid=flip(valid).reshape(F, R), log_w=g.log_w, coalesced=coalesced)


def near_threshold(ref, iou_min, near=1e-5):
    """(decisions, skipped) of the association on frame F - 1: forecast_lane_ref.near_threshold's rule."""
    return FL.near_threshold(ref, iou_min, near)


# ---- the cases of tests/test_track_lane_kernel.py (here, so that the CPU test can hold their inputs against the 1 % cap) -----------
# (K, F, N, wide, hw, iou_min): one particle, a wave, a wave boundary, the whole workgroup; F = 1, 3, 6 stand for lag * T with T in
# {1, 2}; N = 14 is the most a handle takes
CASES = [(K, F, 4, False, (50, 50), 0.5) for K in (1, 2, 5, 64, 65, 256) for F in (1, 3, 6)]
CASES.append((5, 6, 14, True, (50, 50), 0.3))
CASES.append((65, 3, 4, False, (12, 9), 0.7))


def case_id(c):
    return "K{}_F{}_N{}_{}x{}{}".format(c[0], c[1], c[2], c[4][0], c[4][1], "_wide" if c[3] else "")
