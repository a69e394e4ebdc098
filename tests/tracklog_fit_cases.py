"""The inputs of motion calibration's tests (tests/test_tracklog_fit_ref.py on the CPU, tests/test_tracklog_fit_kernel.py on the GPU):
logs of tests/tracklog_cases.py and a few hand-made ones, each with a grid of candidates and a ``burn``.

The cases are the smallest at which the kernel can go wrong (``CASES``, by name).  From tracklog_cases, each as ``<base>_2x2_b0``,
``<base>_2x2_b2``, ``<base>_3x1_b0`` and ``<base>_3x1_b2`` (the grid's size and ``burn``):
  a  the ring wraps;                         e  (N, C, L, lag) = (1, 1, 4, 4);
  f  (14, 64, 16, 16), wide, the log younger than the window;
  g  state 3 inside a span;                  h  the four-frame gap: n_gap > 0;
  i  a track seen once: no term, zero sums;  j  the empty lane.
Beside them:
  p    a's log with C = 5 and a 16 x 16 grid: 2 C = 10 does not divide 256 -- 25 candidates a round, six threads idle, the last
       round partly filled;
  w    two lanes of f's log with C = 64 and a 16 x 16 grid: two candidates a round, eight rounds, 256 candidates a lane;
  l    lag 200 of L = 256, C = 2, two lanes, hand-made: seven staged blocks of 32 frames, the last one of eight;
  bad  one column with an infinite box word: from there on its terms are not counted (skipped > 0) and the sums stay finite;
  sim  the recovery case: 8 lanes, N = 2, C = 4, L = lag = 32, constant-velocity tracks with white acceleration, true (q, r) =
       (1.0, 0.25), 15 % of the frames unseen, one fixed seed, a hand-made log with constant ids, the default 8 x 8 grid around
       (0.25, 1.0): the minimum must be the true node."""
import collections
import functools

import numpy as np

from tests import tracklog_cases as TC
from tests import tracklog_fit_ref as FR
from tests import tracklog_ref as R

V0_VAR = TC.V0_VAR
GRIDS = {"2x2": ((0.25, 1.0), (1.0, 0.25)), "3x1": ((0.0625, 0.25, 4.0), (1.0,))}
GRID16 = tuple(0.01 * 2.0 ** k for k in range(16))
DEFAULT_GRID = (tuple(0.25 * 4.0 ** k for k in range(-4, 4)), tuple(1.0 * 4.0 ** k for k in range(-4, 4)))
SIM_TRUE, SIM_NODE = (1.0, 0.25), (5, 3)
# (every seed tried -- 1 to 5 and 13 -- recovers the node with 110 to 130 nats to the runner-up.  The fp32 bar of the likelihood at the
# two nodes compared depends on how far the tracks wander -- a term's error is an ulp of the coordinate over S -- and was 0.07 to 0.18
# nats over those seeds; tests/test_tracklog_fit_ref.py asserts the margin is 1000 times it, which seeds 1 to 5 meet and seed 13
# misses by a factor of 1.4.  The seed is part of the case, as the offsets of tracklog_score_cases are: one that misses is replaced)
SIM_SEED = 1
BLOCK = 32                                    # the frames the kernel stages at a time (sqair_lane.hip: SQ_FIT_FRAMES)

Case = collections.namedtuple("Case", "name base q_grid r_grid burn")
Inputs = collections.namedtuple("Inputs", "N C L lag wide log solve slot q_grid r_grid burn")
CASES = collections.OrderedDict()
for _base in "aefghij":
    for _g, (_q, _r) in GRIDS.items():
        for _burn in (0, 2):
            _n = "{}_{}_b{}".format(_base, _g, _burn)
            CASES[_n] = Case(_n, _base, _q, _r, _burn)
for _c in (Case("p", "p", GRID16, GRID16, 0), Case("w", "w", GRID16, GRID16, 1), Case("l", "l", *GRIDS["2x2"], 2),
           Case("bad", "bad", *GRIDS["2x2"], 0), Case("sim", "sim", *DEFAULT_GRID, 2)):
    CASES[_c.name] = _c


def hand_log(ids, box, L):
    """A log of L records fed the frames ``ids`` [T, B, N] (-1: the slot is absent) and ``box`` [T, B, N, 4] in one pass, every frame
    finite; track_len counts an id's sightings."""
    T, B, N = ids.shape
    seen, length = {}, np.zeros((T, B, N), np.int32)
    for t in range(T):
        for b in range(B):
            for j in range(N):
                if ids[t, b, j] >= 0:
                    seen[b, ids[t, b, j]] = length[t, b, j] = seen.get((b, ids[t, b, j]), 0) + 1
    return R.append(R.new_log(B, L, N), ids.astype(np.int32), length, np.zeros((T, B), np.int32), box.astype(np.float32))


def _tracks(rng, T, B, N, q, r, unseen, v0_sd=4.0, size=10.0):
    """Constant-velocity tracks with white acceleration of variance q, measured with variance r: (ids, box), slot j holding id j,
    absent in a fraction ``unseen`` of the frames."""
    p = rng.uniform(20.0, 80.0, (B, N, 2))
    v = rng.normal(0.0, v0_sd, (B, N, 2))
    ids, box = -np.ones((T, B, N), np.int64), np.zeros((T, B, N, 4))
    for t in range(T):
        if t:
            acc = rng.normal(0.0, np.sqrt(q), (B, N, 2))
            p, v = p + v + 0.5 * acc, v + acc
        z = p + rng.normal(0.0, np.sqrt(r), (B, N, 2))
        on = rng.uniform(size=(B, N)) >= unseen
        ids[t] = np.where(on, np.arange(N)[None, :], -1)
        box[t, ..., :2], box[t, ..., 2:] = z - 0.5 * size, size
    return ids, box


def _shape_and_log(base):
    """(N, C, L, lag, wide, the log {name: array}) of a base."""
    if base in TC.CASES:
        c = TC.CASES[base]
        return c.N, c.C, c.L, c.lag, c.wide, TC.reference(base)[1]
    if base == "p":
        c = TC.CASES["a"]
        return c.N, 5, c.L, c.lag, c.wide, TC.reference("a")[1]
    if base == "w":
        c = TC.CASES["f"]
        return c.N, 64, c.L, 12, c.wide, {k: np.ascontiguousarray(v[:2]) for k, v in TC.reference("f")[1].items()}
    rng = np.random.RandomState({"l": 11, "bad": 12, "sim": SIM_SEED}[base])
    if base == "l":
        return 2, 2, 256, 200, False, hand_log(*_tracks(rng, 230, 2, 2, 0.25, 1.0, 0.2), L=256)
    if base == "bad":
        ids, box = _tracks(rng, 12, 1, 2, 0.25, 1.0, 0.0)
        box[5, 0, 1, 0] = np.inf
        return 2, 2, 12, 12, False, hand_log(ids, box, L=12)
    return 2, 4, 32, 32, False, hand_log(*_tracks(rng, 32, 8, 2, *SIM_TRUE, 0.15), L=32)


@functools.lru_cache(maxsize=None)
def _base(base):
    N, C, L, lag, wide, log = _shape_and_log(base)
    for a in log.values():
        a.setflags(write=False)
    with np.errstate(all="ignore"):   # (bad's infinite word)
        solve = R.smooth(log, lag, C, TC.Q, TC.R_MEAS, TC.V0_VAR)
    return N, C, L, lag, wide, log, solve, FR.slots(log, solve, lag)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """``Inputs`` of a case: the shape, the log, the reference's solve of it (tracklog_ref.Smooth), the slots of its columns, the
    grids and ``burn``.  Made once, never written to."""
    c = CASES[name]
    return Inputs(*_base(c.base), c.q_grid, c.r_grid, c.burn)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference's fit of a case on the reference's own solve: made once, never written to."""
    x = inputs(name)
    return FR.fit(x.log, x.solve.frame_index, x.solve.state, x.slot, x.q_grid, x.r_grid, V0_VAR, x.burn)


# ------------------------------------------------------------------------------------------------ the kernel on caller buffers (GPU)
PARITY_NOTE = ("per case of tests/test_tracklog_fit_kernel.py: the worst fp32 error of a term of each kind -- the fp32 restatement of the "
               "header against float64 (tests/tracklog_fit_ref.py); a sum's bar is four times that times its number of terms --, the "
               "kernel's own worst error of each sum against float64 and the largest bar it was held to, innov's error and bar, and "
               "what the case holds; counts and innov's zero pattern are compared exactly")


def record(section, case, **figures):
    """One case's figures into tracklog_fit_parity.json under SQAIR_PARITY_DIR."""
    import torch
    from sqair_amd import _capi
    from tests.kernel_unit import merge_parity

    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data.setdefault(section, {})[case] = figures
    merge_parity("tracklog_fit_parity.json", lambda: {"note": PARITY_NOTE, "cases": {}, "stream": {}}, update)


def fit_buffers(lag, B, C_, Q, Rn):
    """The fit's outputs, filled with -7 so that every word must be written."""
    import torch
    from sqair_amd import _capi
    return {k: torch.full(shp, -7, dtype=getattr(torch, _capi.field_dtype("SqairTrackLogFit", k)), device="cuda")
            for k, shp in _capi.tracklog_fit_shapes(lag, B, C_, Q, Rn).items()}


def run_fit(lib, h, d, L, table, work, out, lag, C_, N, q_grid, r_grid, burn, v0_var=V0_VAR, stream=None, innov=True):
    """One launch of k_lane_tracklog_fit: device log ``d``, the solve's device outputs ``table`` and ``work``, into ``out``."""
    import ctypes as C
    import torch
    from sqair_amd import _capi
    B = d["count"].shape[0]
    tab = _capi.SqairTrackLogOut(**{n: table[n].data_ptr() for n in _capi.TRACKLOG_FIT_TABLE})
    ptr = {n: t.data_ptr() for n, t in out.items() if innov or n != "innov"}
    f = _capi.tracklog_fit_struct(q_grid, r_grid, v0_var, burn, **ptr)
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = lib.sqair_lane_tracklog_fit(h, C.byref(TC.log_struct(d, L)), C.byref(tab), work.data_ptr(), C.byref(f), lag, C_, N, B, s)
    assert rc == 0, lib.sqair_last_error(h)
