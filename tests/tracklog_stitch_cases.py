"""The inputs of track log stitching's tests (tests/test_tracklog_stitch_ref.py on the CPU, tests/test_tracklog_stitch_kernel.py on the
GPU): hand-made logs of constant-velocity objects, 10 x 10 boxes, measured with a noise of 0.3 px (fixed seeds), whose ids change the
way a causal tracker's do -- and beside each the PLAIN log, the same frames never relabelled: every fragment under its object's first
id.  The motion's default scalars, gate 3.5, max_gap = lag unless said.

The cases are the smallest at which the kernel can go wrong (``CASES``, by name); B = 3 lanes, N = 2, C = 4, L = 32, lag = 24 unless said:
  relabel            one id change across a 4-frame drop-out, track_len restarting at 1; a steady track beside it; two at once;
  relabel_chain      a -> b -> c, one of the changes between consecutive frames (gap 0);
  crossing           two tracks end and two are born where the nearest newborn by position is the other object's;
  refused_links      B = 4, max_gap = 3, one lane each: d2 beyond the gate, gap above max_gap, a successor with len0 > 1, overlapping
                     spans: no link anywhere;
  invalid_inside     max_gap = 3: non-finite frames inside the bridged gap (not counted, not stepped, state 3), at its edges, and inside
                     a fragment;
  young_and_wrapped  a lane with count < lag, a lane with count > L (the ring wraps; the predecessor was born before the window);
  dropped_root       more ids than C: a chain whose oldest fragments are not kept, a kept newborn whose predecessor is not;
  nonfinite          a NaN box word at a fragment's last sighting, and inside a fragment: no link from there;
  empty              a lane without ids between two that have some;
  limit              B = 2, N = 16, C = 64, L = lag = 64, max_gap = 8: 32 relabelled pairs a lane, the slots time-shared: the assignment
                     at its limits;
  dropout            B = 1, N = 1: the README's moving drop-out, 3 px a frame, unseen for 12 frames, run through the identity's
                     reference with identity_max_age = 10 as tests/tracklog_cases.py's ``identity_run`` runs its scenes (that function
                     takes its own scenes only): the returning object gets a fresh lane_id.  With the object's true boxes as truth,
                     G = 1."""
import collections
import functools

import numpy as np

from tests import motion_cases as MC
from tests import motion_ref as MR
from tests import tracklog_cases as TC
from tests import tracklog_ref as R
from tests import tracklog_stitch_ref as SR

Q, R_MEAS, V0_VAR = TC.Q, TC.R_MEAS, TC.V0_VAR
GATE = 3.5
NOISE = 0.3
SIZE = 10.0
IOU_MIN = 0.5

Obj = collections.namedtuple("Obj", "slot p0 v segs")            # segs: [(first, last)] the frames the object is seen in, per fragment
Case = collections.namedtuple("Case", "name N C L lag gate max_gap log plain truth")
Ref = collections.namedtuple("Ref", "solve stitch plain")
NAMES = ("relabel", "relabel_chain", "crossing", "refused_links", "invalid_inside", "young_and_wrapped", "dropped_root", "nonfinite",
         "empty", "limit", "dropout")
BITS = ("relabel", "relabel_chain", "crossing", "limit")          # stitched == the solve of the plain log, bit for bit


def _lane(objs, T, N, L, seed, invalid=(), len_start=None, poke=()):
    """(the log of ONE lane, its plain twin) of ``objs`` over T frames: fragment ids in the order of (birth frame, slot), track_len
    counting an id's sightings (from ``len_start[id]`` + 1), frames ``invalid`` non-finite, ``poke``: (frame, slot, word, value)."""
    rng = np.random.RandomState(seed)
    births = sorted((s[0], o.slot, i, k) for i, o in enumerate(objs) for k, s in enumerate(o.segs))
    ids = {(i, k): n for n, (_, _, i, k) in enumerate(births)}
    out = []
    noise = rng.normal(0.0, NOISE, (T, len(objs), 2))
    for plain in (False, True):
        lane_id, track_len = -np.ones((T, 1, N), np.int32), -np.ones((T, 1, N), np.int32)
        box = np.zeros((T, 1, N, 4), np.float32)
        seen = dict(len_start or {})
        for t in range(T):
            for i, o in enumerate(objs):
                for k, (lo, hi) in enumerate(o.segs):
                    if lo <= t <= hi:
                        tid = ids[i, 0 if plain else k]
                        seen[tid] = seen.get(tid, 0) + 1
                        lane_id[t, 0, o.slot], track_len[t, 0, o.slot] = tid, seen[tid]
                        centre = np.asarray(o.p0, np.float64) + np.asarray(o.v, np.float64) * t + noise[t, i]
                        box[t, 0, o.slot, :2], box[t, 0, o.slot, 2:] = centre - 0.5 * SIZE, SIZE
        for t, j, w, v in poke:
            box[t, 0, j, w] = v
        best_row = np.zeros((T, 1), np.int32)
        best_row[list(invalid)] = -1
        out.append(R.append(R.new_log(1, L, N), lane_id, track_len, best_row, box))
    return out


def _stack(lanes):
    """The lanes' (log, plain) pairs as one (log, plain) of B lanes."""
    return tuple({k: np.concatenate([l[i][k] for l in lanes]) for k in R.FIELDS} for i in (0, 1))


def _relabel_lane(seed, T=24, N=2, L=32):
    return _lane([Obj(0, (10.0 + seed, 20.0), (1.5, -0.5), [(0, 9), (14, T - 1)])], T, N, L, seed)


def _limit_lane(seed):
    rng = np.random.RandomState(100 + seed)
    objs = []
    for half in (0, 1):
        for j in range(16):
            e1, g = int(rng.randint(10, 14)), int(rng.randint(2, 7))
            p0 = (100.0 * (j // 4) + 50.0 * half, 100.0 * (j % 4) + 50.0 * half)
            objs.append(Obj(j, p0, tuple(rng.uniform(-2.0, 2.0, 2)), [(32 * half, 32 * half + e1), (32 * half + e1 + g + 1, 32 * half + 31)]))
    return _lane(objs, 64, 16, 64, 200 + seed)


def _dropout():
    """(log, plain, truth) of the moving drop-out: seen in frames 0-5 and 18-23, unseen for 12."""
    T = 24
    seen = [t < 6 or t >= 18 for t in range(T)]
    true = np.array([(10.0 + 3.0 * t, 20.0) for t in range(T)])
    x = MC.scenario(true, seen)
    run = MR.scenario_run(x, 2.0, 10, MC.SCALARS)
    lane_id, track_len = run.lane_id.astype(np.int32), run.track_len.astype(np.int32)
    assert sorted(set(lane_id[lane_id >= 0].tolist())) == [0, 1], "the identity re-identified the object: no fragments to stitch"
    log = R.append(R.new_log(1, 32, 1), lane_id, track_len, x["best_row"].astype(np.int32), x["box"].astype(np.float32))
    plain = R.append(R.new_log(1, 32, 1), np.where(lane_id >= 0, 0, -1).astype(np.int32), np.cumsum(lane_id >= 0, 0).astype(np.int32),
                     x["best_row"].astype(np.int32), x["box"].astype(np.float32))
    tb = np.zeros((T, 1, 1, 4), np.float32)
    tb[:, 0, 0, :2], tb[:, 0, 0, 2:] = true - 5.0, 10.0
    truth = dict(truth_box=tb, truth_present=np.ones((T, 1, 1), np.int32), truth_valid=np.ones((T, 1), np.int32))
    return log, plain, truth


def _build(name):
    N, C, L, lag, max_gap, truth = 2, 4, 32, 24, 24, None
    T = 24
    if name == "relabel":
        lanes = [_relabel_lane(1),
                 _lane([Obj(0, (30.0, 5.0), (-1.0, 2.0), [(0, 11), (16, 23)]), Obj(1, (40.0, 40.0), (0.2, 0.1), [(0, 23)])], T, N, L, 2),
                 _lane([Obj(0, (5.0, 5.0), (2.0, 1.0), [(0, 8), (13, 23)]), Obj(1, (45.0, 90.0), (-1.0, -2.5), [(1, 10), (15, 23)])], T, N, L, 3)]
    elif name == "relabel_chain":
        lanes = [_lane([Obj(0, (10.0, 10.0), (1.0, 2.0), [(0, 7), (8, 15), (19, 23)])], T, N, L, 4),
                 _lane([Obj(0, (50.0, 10.0), (-1.5, 0.5), [(0, 5), (9, 14), (15, 23)])], T, N, L, 5),
                 _lane([Obj(0, (20.0, 70.0), (0.5, -2.0), [(0, 7), (8, 15), (20, 23)]), Obj(1, (80.0, 15.0), (0.1, 0.3), [(2, 23)])], T, N, L, 6)]
    elif name == "crossing":
        lanes = [_lane([Obj(0, (20.0, 40.0), (0.0, 2.0), [(0, 9), (14, 23)]), Obj(1, (20.0, 88.0), (0.0, -2.0), [(0, 9), (14, 23)])], T, N, L, 7),
                 _lane([Obj(0, (40.0, 20.0), (2.0, 0.0), [(0, 9), (14, 23)]), Obj(1, (88.0, 20.0), (-2.0, 0.0), [(0, 9), (14, 23)])], T, N, L, 8),
                 _lane([Obj(0, (40.0, 40.0), (2.0, 2.0), [(0, 9), (14, 23)]), Obj(1, (88.0, 88.0), (-2.0, -2.0), [(0, 9), (14, 23)])], T, N, L, 9)]
    elif name == "refused_links":
        max_gap = 3
        lanes = [_lane([Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 9)]), Obj(1, (40.0, 20.0), (1.5, -0.5), [(12, 23)])], T, N, L, 10),
                 _lane([Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 9), (15, 23)])], T, N, L, 11),
                 _lane([Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 9), (12, 23)])], T, N, L, 12, len_start={1: 3}),
                 _lane([Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 12)]), Obj(1, (11.0, 20.0), (1.5, -0.5), [(10, 23)])], T, N, L, 13)]
    elif name == "invalid_inside":
        max_gap = 3
        one = [Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 9), (15, 23)])]
        lanes = [_lane(one, T, N, L, 14, invalid=(11, 12)), _lane(one, T, N, L, 15, invalid=(10, 14)), _lane(one, T, N, L, 16, invalid=(5, 12, 13))]
    elif name == "young_and_wrapped":
        lanes = [_lane([Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 5), (9, 14)])], 15, N, L, 17),
                 _lane([Obj(0, (10.0, 20.0), (1.0, 0.5), [(0, 12), (14, 25), (30, 39)])], 40, N, L, 18),
                 _relabel_lane(19)]
    elif name == "dropped_root":
        lanes = [_lane([Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 2), (4, 6), (8, 10), (12, 14), (16, 18), (20, 23)])], T, N, L, 20),
                 _lane([Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 7), (10, 23)]), Obj(1, (70.0, 60.0), (-1.0, 1.0), [(0, 4), (7, 12), (15, 23)])],
                       T, N, L, 21),
                 _relabel_lane(22)]
    elif name == "nonfinite":
        one = [Obj(0, (10.0, 20.0), (1.5, -0.5), [(0, 9), (14, 23)])]
        lanes = [_lane(one, T, N, L, 23, poke=[(9, 0, 0, np.nan)]), _relabel_lane(24), _lane(one, T, N, L, 25, poke=[(5, 0, 1, np.nan)])]
    elif name == "empty":
        lanes = [_relabel_lane(26), _lane([], T, N, L, 27), _relabel_lane(28)]
    elif name == "limit":
        N, C, L, lag, max_gap = 16, 64, 64, 64, 8
        lanes = [_limit_lane(0), _limit_lane(1)]
    elif name == "dropout":
        N = 1
        log, plain, truth = _dropout()
        lanes = None
    if lanes is not None:
        log, plain = _stack(lanes)
    for d in (log, plain) + ((truth,) if truth else ()):
        for a in d.values():
            a.setflags(write=False)
    return Case(name, N, C, L, lag, GATE, max_gap, log, plain, truth)


@functools.lru_cache(maxsize=None)
def make(name):
    """The ``Case``: its shape and scalars, the log {name: array}, its plain twin, the truth in window order (dropout).  Made once,
    never written to."""
    return _build(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """``Ref``: the reference's solve of the case's log, its stitch of that, and its solve of the plain log.  Made once."""
    c = make(name)
    with np.errstate(all="ignore"):   # (nonfinite's NaN words)
        sm = R.smooth(c.log, c.lag, c.C, Q, R_MEAS, V0_VAR)
        plain = R.smooth(c.plain, c.lag, c.C, Q, R_MEAS, V0_VAR)
    return Ref(sm, SR.stitch(c.log, sm, c.lag, c.C, Q, R_MEAS, V0_VAR, c.gate, c.max_gap), plain)


def table_of(table):
    """What the scorer reads of a ``tracklog_ref.Smooth``: the fp32 restatement's words stand for filt and smooth."""
    return dict(track_id=table.track_id, frame_index=table.frame_index, state=table.state, size=table.size, filt=table.filt32,
                smooth=table.smooth32)


# ------------------------------------------------------------------------------------------------ the kernel on caller buffers (GPU)
PARITY_NOTE = ("per case of tests/test_tracklog_stitch_kernel.py: the worst fp32 error of a candidate's d2 -- the fp32 restatement of the "
               "header against float64 (tests/tracklog_stitch_ref.py) --, the bar link_d2 was held to (four times it), the kernel's own "
               "worst error of link_d2, the bars of the stitched filt and smooth (tests/tracklog_ref.py: bars) and the kernel's own "
               "errors, and what the case holds; every integer output is compared exactly")


def record(section, case, **figures):
    """One case's figures into tracklog_stitch_parity.json under SQAIR_PARITY_DIR."""
    import torch
    from sqair_amd import _capi
    from tests.kernel_unit import merge_parity

    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data.setdefault(section, {})[case] = figures
    merge_parity("tracklog_stitch_parity.json", lambda: {"note": PARITY_NOTE, "cases": {}, "stream": {}}, update)


def stitch_buffers(lib, lag, B, C_, N):
    """(the stitched table, work_out, the link outputs), every one filled with -7 so that every word must be written."""
    import torch
    from sqair_amd import _capi
    out, work_out = TC.solve_buffers(lib, lag, B, C_, N)
    work_out.fill_(-7)
    links = {k: torch.full(shp, -7, dtype=getattr(torch, _capi.field_dtype("SqairTrackLogStitch", k)), device="cuda")
             for k, shp in _capi.tracklog_stitch_shapes(B, C_).items()}
    return out, work_out, links


def run_stitch(lib, h, d, L, table, work, out, work_out, links, lag, C_, N, gate, max_gap, scalars=(Q, R_MEAS, V0_VAR), stream=None):
    """One launch of k_lane_tracklog_stitch: device log ``d``, the solve's device outputs ``table`` and ``work``, into ``out``,
    ``work_out`` and ``links``."""
    import ctypes as C
    import torch
    from sqair_amd import _capi
    B = d["count"].shape[0]
    tab = _capi.SqairTrackLogOut(**{n: t.data_ptr() for n, t in table.items()})
    o = _capi.SqairTrackLogOut(**{n: t.data_ptr() for n, t in out.items()})
    st = _capi.SqairTrackLogStitch(gate=gate, max_gap=max_gap, **{n: t.data_ptr() for n, t in links.items()})
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = lib.sqair_lane_tracklog_stitch(h, C.byref(TC.log_struct(d, L)), C.byref(tab), work.data_ptr(), lag, C_, N, B, *scalars, C.byref(st),
                                        C.byref(o), work_out.data_ptr(), s)
    assert rc == 0, lib.sqair_last_error(h)
