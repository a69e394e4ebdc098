"""The reference of the track log (include/sqair_hip.h: sqair_set_tracklog, the track log paragraph), restated from the header and not
from the kernels.  NumPy, plain loops.

``append`` is point A in integers and 32-bit words.  ``smooth`` is points 1 to 5: the window and the columns in integers, the forward
filter and the Rauch-Tung-Striebel pass in float64 -- only the box words are fp32 --, and beside every float64 state the fp32
RESTATEMENT (numpy ``float32``, the header's operations in the header's order, ``motion_ref._fma`` where the header says ``fmaf``).
The solve makes no threshold decision, so the restatement never leaves the float64 run's path: what it differs by from float64 is the
measured fp32 error of ``filt`` and ``smooth``, per lane in ``Smooth.err``; ``bars`` is four times the largest of it (the project's
rule, as ``motion_ref.bars``)."""
import collections

import numpy as np

from tests.motion_ref import _fma

FIELDS = ("count", "log_valid", "log_id", "log_len", "log_box")
OUTSIDE, SEEN, GAP, INVALID = 0, 1, 2, 3

Smooth = collections.namedtuple("Smooth", "track_id n_tracks len0 frame_index state size filt smooth filt32 smooth32 err")


def new_log(B, L, N):
    """The caller's start: zeros."""
    return dict(count=np.zeros(B, np.int64), log_valid=np.zeros((B, L), np.int32), log_id=np.zeros((B, L, N), np.int32),
                log_len=np.zeros((B, L, N), np.int32), log_box=np.zeros((B, L, N, 4), np.float32))


def append(log, lane_id, track_len, best_row, box):
    """Point A for one pass of T frames: a new log {name: array}, the given one untouched.  lane_id, track_len [T, B, N] int32,
    best_row [T, B], box [T, B, N, 4] float32 (copied as words)."""
    log = {k: np.array(v) for k, v in log.items()}
    T, B = np.asarray(best_row).shape
    L = log["log_valid"].shape[1]
    words = log["log_box"].view(np.uint32)
    for b in range(B):
        for t in range(T):
            rec = int((int(log["count"][b]) + t) % L)
            log["log_valid"][b, rec] = 0 if best_row[t, b] == -1 else 1
            log["log_id"][b, rec] = lane_id[t, b]
            log["log_len"][b, rec] = track_len[t, b]
            words[b, rec] = np.asarray(box[t, b], np.float32).view(np.uint32)
        log["count"][b] += T
    return log


# ---- the filter's statements, in ``ft`` (np.float64, or np.float32 with _fma where the header says fmaf) --------------------------
def _fmaf(ft):
    return _fma if ft is np.float32 else (lambda a, b, c: a * b + c)


def start(z, r, v0_var, ft):
    return [ft(z), ft(0), ft(r), ft(0), ft(v0_var)]


def predict(k, q, r, ft):
    """The motion paragraph's P on (p, v, Ppp, Ppv, Pvv); returns (the predicted state, S)."""
    p, v, a, b, c = k
    q = ft(q)
    npp = ((a + ft(2) * b) + c) + ft(0.25) * q
    return [p + v, v, npp, (b + c) + ft(0.5) * q, c + q], npp + ft(r)


def update(k, S, z, ft):
    """The motion paragraph's U on the predicted state."""
    fma = _fmaf(ft)
    p, v, a, b, c = k
    y, k0, k1 = ft(z) - p, a / S, b / S
    return [fma(k0, y, p), fma(k1, y, v), (ft(1) - k0) * a, (ft(1) - k0) * b, fma(-k1, b, c)]


def rts(k, nxt, q, r, ft):
    """Point 4: the smoothed state of a stepped frame from its filtered state ``k`` and the next stepped frame's smoothed ``nxt``."""
    fma = _fmaf(ft)
    p, v, a, b, c = k
    ps1, vs1, as1, bs1, cs1 = nxt
    (pm, _, am, bm, cm), _ = predict(k, q, r, ft)
    det, m00, m10 = fma(am, cm, -(bm * bm)), a + b, b + c
    g00, g01 = fma(m00, cm, -(b * bm)) / det, fma(b, am, -(m00 * bm)) / det
    g10, g11 = fma(m10, cm, -(c * bm)) / det, fma(c, am, -(m10 * bm)) / det
    dp, dv, da, db, dc = ps1 - pm, vs1 - v, as1 - am, bs1 - bm, cs1 - cm
    ps, vs = fma(g01, dv, fma(g00, dp, p)), fma(g11, dv, fma(g10, dp, v))
    e00, e01 = fma(g01, db, g00 * da), fma(g01, dc, g00 * db)
    e10, e11 = fma(g11, db, g10 * da), fma(g11, dc, g10 * db)
    return [ps, vs, fma(e01, g01, fma(e00, g00, a)), fma(e01, g11, fma(e00, g10, b)), fma(e11, g11, fma(e10, g10, c))]


def window(log, b, lag):
    """Point 1 for lane b: (frame_index [lag] int64, record [lag] (-1: none), counts [lag] bool)."""
    L = log["log_valid"].shape[1]
    g = int(log["count"][b]) - lag + np.arange(lag, dtype=np.int64)
    rec = np.where(g >= 0, g % L, -1)
    counts = np.array([r >= 0 and log["log_valid"][b, r] != 0 for r in rec], bool)
    return np.where(g >= 0, g, -1), rec, counts


def smooth(log, lag, C, q, r, v0_var):
    """Points 1 to 5 on a log {name: array}; the scalars are taken as the fp32 values the call is handed."""
    q, r, v0_var = (float(np.float32(v)) for v in (q, r, v0_var))
    B, L, N = log["log_id"].shape
    track_id, len0 = -np.ones((B, C), np.int32), -np.ones((B, C), np.int32)
    n_tracks, frame_index = np.zeros(B, np.int32), np.zeros((lag, B), np.int64)
    state, size = np.zeros((lag, B, C), np.int32), np.zeros((lag, B, C, 2), np.float32)
    filt, sm = np.zeros((lag, B, C, 2, 5)), np.zeros((lag, B, C, 2, 5))
    filt32, sm32 = np.zeros((lag, B, C, 2, 5), np.float32), np.zeros((lag, B, C, 2, 5), np.float32)
    err = dict(filt=np.zeros(B), smooth=np.zeros(B))
    for b in range(B):
        frame_index[:, b], rec, counts = window(log, b, lag)
        ids = sorted({int(i) for f in range(lag) if counts[f] for i in log["log_id"][b, rec[f]] if i >= 0})        # 2
        n_tracks[b] = len(ids)
        kept = ids[-C:]
        track_id[b, :len(kept)] = kept
        for c, tid in enumerate(kept):
            slot = [int(np.flatnonzero(log["log_id"][b, rec[f]] == tid)[0]) if counts[f] and (log["log_id"][b, rec[f]] == tid).any() else -1
                    for f in range(lag)]
            seen = [f for f in range(lag) if slot[f] >= 0]
            f0, f1 = seen[0], seen[-1]
            len0[b, c] = log["log_len"][b, rec[f0], slot[f0]]
            for ax in range(2):
                for ft, out_f, out_s in ((np.float64, filt, sm), (np.float32, filt32, sm32)):
                    k, stepped = None, []
                    for f in range(f0, f1 + 1):                                                                      # 3
                        if not counts[f]:
                            state[f, b, c] = INVALID
                            continue
                        j = slot[f]
                        if j >= 0:
                            bx = log["log_box"][b, rec[f], j]
                            z = _fmaf(ft)(ft(0.5), ft(bx[2 + ax]), ft(bx[ax]))
                            size[f, b, c, ax] = bx[2 + ax]
                        else:
                            size[f, b, c, ax] = size[stepped[-1], b, c, ax]
                        if f == f0:
                            k = start(z, r, v0_var, ft)
                        else:
                            k, S = predict(k, q, r, ft)
                            if j >= 0:
                                k = update(k, S, z, ft)
                        state[f, b, c] = SEEN if j >= 0 else GAP
                        out_f[f, b, c, ax] = k
                        stepped.append(f)
                    nxt = None
                    for f in reversed(stepped):                                                                      # 4
                        k = [ft(v) for v in out_f[f, b, c, ax]]
                        nxt = k if nxt is None else rts(k, nxt, q, r, ft)
                        out_s[f, b, c, ax] = nxt
        err["filt"][b] = float(np.abs(filt32[:, b] - filt[:, b]).max())
        err["smooth"][b] = float(np.abs(sm32[:, b] - sm[:, b]).max())
    return Smooth(track_id, n_tracks, len0, frame_index, state, size, filt, sm, filt32, sm32, err)


def bars(err):
    """The bars of filt and smooth: four times the largest error of the fp32 restatement over the lanes."""
    return {n: 4.0 * float(err[n].max()) for n in ("filt", "smooth")}


# ---- an independent derivation: the same posterior solved directly ---------------------------------------------------------------
def direct_means(zs, q, r, v0_var):
    """The smoothed means [n, 2] = (p, v) of one axis of one track over n consecutive stepped frames, ``zs`` its measurements (None
    in a gap; zs[0] is the first sighting), by a direct solve of the same linear-Gaussian posterior: the weighted normal equations
    of the prior x_0 ~ N((z_0, 0), diag(r, v0_var)), the dynamics and the measurements z_k = p_k + e, e ~ N(0, r), of the later
    sightings, solved with numpy.linalg.solve.  No recursion.  The process noise Q = q [[1/4, 1/2], [1/2, 1]] = q g g^T, g = (1/2, 1),
    has rank one, so the block-tridiagonal form in the states alone, which needs Q^-1, does not exist; the equations are written in
    x_0 and the scalar white accelerations a_k ~ N(0, q) instead, x_{k+1} = F x_k + g a_k, which is the same model."""
    n = len(zs)
    F = np.array([[1.0, 1.0], [0.0, 1.0]])
    G = np.array([0.5, 1.0])
    # unknowns: x_0 (2) and a_0 .. a_{n-2}; x_k = F^k x_0 + sum_i F^(k-1-i) G a_i is linear in them
    m = 2 + (n - 1)
    rows = []
    Fk = [np.linalg.matrix_power(F, k) for k in range(n)]

    def state_row(k):
        A = np.zeros((2, m))
        A[:, :2] = Fk[k]
        for i in range(k):
            A[:, 2 + i] = Fk[k - 1 - i] @ G
        return A
    H, y, w = [], [], []
    X0 = state_row(0)
    H += [X0[0], X0[1]]; y += [zs[0], 0.0]; w += [1.0 / r, 1.0 / v0_var]
    for i in range(n - 1):
        e = np.zeros(m); e[2 + i] = 1.0
        H.append(e); y.append(0.0); w.append(1.0 / q)
    for k in range(1, n):
        if zs[k] is not None:
            H.append(state_row(k)[0]); y.append(zs[k]); w.append(1.0 / r)
    H, y, w = np.array(H), np.array(y), np.array(w)
    theta = np.linalg.solve(H.T @ (w[:, None] * H), H.T @ (w * y))
    return np.array([state_row(k) @ theta for k in range(n)])
