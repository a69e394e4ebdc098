"""NumPy reference of the track history (include/sqair_hip.h: sqair_set_history / sqair_history_trace): a recorder of per-step
outputs and import maps, and the tracer over them.  Plain Python, no GPU; the reference of tests/test_history.py.

A step is a dict: ``parent`` [R] (the map the step imported through; -1 or out of range = the row started fresh), ``t0`` [R] (the
row's frame counter at the step's first frame), ``where`` [T, R, N, 4], ``presence``, ``obj_id`` [T, R, N] and optionally ``what``
[T, R, N, n_what] and ``log_w`` [T, R].  Values are copied as they are (NaNs and signed zeros included: compare bit patterns)."""
import numpy as np

FIELDS = ("where", "presence", "obj_id", "what", "log_w")


def norm_map(m, R):
    """A source map as the state import reads it: -1 for every index outside [0, R)."""
    m = np.asarray(m, dtype=np.int64)
    return np.where((m >= 0) & (m < R), m, -1)


class Recorder(object):
    """Keeps every step pushed and the rows' frame counters: a fresh row starts at 0, an imported one continues its source's."""

    def __init__(self, R):
        self.R = int(R)
        self.steps = []
        self.counter = np.zeros(self.R, dtype=np.int64)   # after the last step

    def push(self, parent, **outputs):
        parent = norm_map(parent, self.R)
        T = np.asarray(outputs["where"]).shape[0]
        t0 = np.where(parent >= 0, self.counter[np.maximum(parent, 0)], 0)
        self.counter = t0 + T
        step = dict(parent=parent, t0=t0)
        for k, v in outputs.items():
            assert k in FIELDS, k
            step[k] = np.array(v, copy=True)
        self.steps.append(step)
        return step


def trace(steps, L, lag, K, start_rows=None, max_tracks=None):
    """Traces the last ``lag`` of ``steps`` (all steps pushed so far, oldest first; a ring of ``L`` keeps the last L of them).
    ``start_rows`` None: a = r; else a = start_rows[r] (-1 / out of range: an empty path).  Frames oldest -> newest."""
    assert 1 <= lag <= L
    kept = steps[-L:]
    if kept:
        first = kept[0]
        T, R, N = first["presence"].shape
    else:
        raise ValueError("trace() needs at least one step to know the shapes; use empty_trace()")
    return _trace(kept, T, R, N, lag, K, start_rows, max_tracks,
                  {k: first[k].shape[3:] if k in ("where", "what") else () for k in FIELDS if k in first},
                  {k: first[k].dtype for k in FIELDS if k in first})


def empty_trace(T, R, N, n_what, lag, K, fields=FIELDS, max_tracks=None):
    """The trace of a ring nothing was pushed into."""
    tails = {k: ((4,) if k == "where" else (n_what,) if k == "what" else ()) for k in fields}
    return _trace([], T, R, N, lag, K, None, max_tracks, tails, {k: np.float32 for k in fields})


def _trace(kept, T, R, N, lag, K, start_rows, max_tracks, tails, dtypes):
    F, B = lag * T, R // K
    out = dict(valid=np.zeros((F, R), np.int32), frame_index=np.full((F, R), -1, np.int32),
               ancestor_row=np.full((lag, R), -1, np.int32), unique_ancestors=np.zeros((lag, B), np.int32))
    for k, tail in tails.items():
        mid = (N,) if k != "log_w" else ()
        out[k] = np.zeros((F, R) + mid + tuple(tail), dtypes[k])
    a = np.arange(R, dtype=np.int64) if start_rows is None else norm_map(start_rows, R)
    for j in range(lag):               # j steps back from the newest
        i = lag - 1 - j
        if j >= len(kept):
            a = np.full(R, -1, dtype=np.int64)
        out["ancestor_row"][i] = a
        for b in range(B):
            lane = a[b * K:(b + 1) * K]
            out["unique_ancestors"][i, b] = len(set(lane[lane >= 0].tolist()))
        if j >= len(kept):
            continue
        step = kept[len(kept) - 1 - j]
        ok = a >= 0
        src = np.maximum(a, 0)
        for t in range(T):
            f = i * T + t
            out["valid"][f] = ok
            out["frame_index"][f] = np.where(ok, step["t0"][src] + t, -1)
            for k in tails:
                v = step[k][t][src]
                v = v.copy()
                v[~ok] = 0
                out[k][f] = v
        a = np.where(ok, norm_map(step["parent"], R)[src], -1)
    if max_tracks is not None:
        out.update(track_table(out["presence"], out["obj_id"], out["where"], out["valid"], max_tracks))
    return out


def track_table(presence, obj_id, where, valid, M):
    """Slots -> tracks: per row the ids present (presence == 1) in a valid frame, ascending, the first M."""
    F, R, N = presence.shape
    track_id = np.full((R, M), -1, np.int32)
    n_tracks = np.zeros(R, np.int32)
    present = np.zeros((F, R, M), np.float32)
    twhere = np.zeros((F, R, M, 4), where.dtype)
    for r in range(R):
        on = (presence[:, r] == 1) & (valid[:, r, None] != 0)          # [F, N]
        ids = sorted(set(int(v) for v in obj_id[:, r][on].tolist()))
        n_tracks[r] = len(ids)
        for m, oid in enumerate(ids[:M]):
            track_id[r, m] = oid
            for f in range(F):
                for n in range(N):
                    if on[f, n] and int(obj_id[f, r, n]) == oid:
                        present[f, r, m] = 1
                        twhere[f, r, m] = where[f, r, n]
                        break
    return dict(track_id=track_id, n_tracks=n_tracks, track_present=present, track_where=twhere)


def same_bits(a, b):
    """Equal shapes, dtypes' sizes and bit patterns."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()
