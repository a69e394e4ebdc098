"""The inputs of the track log's tests (tests/test_tracklog_ref.py on the CPU, tests/test_tracklog_kernel.py on the GPU): the scenes
of tests/motion_cases.py run through tests/motion_ref.py's ``identity``, so that the ids, the lengths and the boxes a log is fed are
real ones -- fast and slow objects, moving drop-outs, best-row switches, births into a full table --, at most 8 lanes of T = 12
frames.  Lanes LANES of a scene are taken; among them motion_cases' non-finite lane (from frame 3 on, lane NAN here) and its empty
lane (lane EMPTY here).

The cases are the smallest at which the kernels can go wrong (``CASES``, by name):
  a  (N, C, L, lag) = (4, 8, 8, 8), T = 12 in passes of 5 + 7: the ring wraps;
  b  lag 8 with count 3: frames without a record;
  c  lag 5 < count;
  d  C = 2 with more distinct ids than that: the newest are kept, n_tracks is above C;
  e  (1, 1, 4, 4);
  f  (14, 64, 16, 16): wide, the log younger than the window;
  g  a lane with non-finite frames inside a span (state 3);
  h  the README's moving drop-out: a four-frame gap inside a span;
  i  a track seen once: smooth == filt == the start;
  j  the empty lane, alone."""
import collections
import functools

import numpy as np

from tests import motion_cases as MC
from tests import motion_ref as MR
from tests import tracklog_ref as R

LANES = (0, 1, 2, 3, 4, 5, MC.NAN_LANE, MC.EMPTY_LANE)
NAN, EMPTY = 6, 7
T = MC.T
Q, R_MEAS, V0_VAR = MC.Q, MC.R_MEAS, MC.V0_VAR
GAP_LANE, GAP_FRAMES = 2, (5, 6)            # case g: these frames of this lane are non-finite, the ones around them are not

Case = collections.namedtuple("Case", "name N C L lag passes wide scene")
CASES = collections.OrderedDict((c.name, c) for c in (
    Case("a", 4, 8, 8, 8, (5, 7), False, 0),
    Case("b", 4, 8, 8, 8, (3,), False, 0),
    Case("c", 4, 8, 8, 5, (12,), False, 0),
    Case("d", 4, 2, 16, 12, (12,), False, 0),
    Case("e", 1, 1, 4, 4, (12,), False, 2),
    Case("f", 14, 64, 16, 16, (12,), True, 3),
    Case("g", 4, 8, 16, 12, (12,), False, "gap"),
    Case("h", 1, 4, 16, 11, (11,), False, "dropout"),
    Case("i", 1, 4, 16, 12, (12,), False, "once"),
    Case("j", 4, 8, 8, 8, (12,), False, "empty"),
))
INPUTS = ("lane_id", "track_len", "best_row", "box")


@functools.lru_cache(maxsize=None)
def identity_run(scene):
    """(the identity's inputs {name: array} of the scene, motion_ref's run on them with motion_cases' scalars)."""
    kw = dict(iou_min=MC.IOU_MIN, reid_dist=MC.REID_DIST, reid_what=float("inf"), max_age=MC.MAX_AGE, motion=MC.SCALARS)
    if scene == "dropout":
        x = MC.moving_dropout()[0]
        return x, MR.scenario_run(x, 2.0, 10, MC.SCALARS)
    if scene == "once":
        x = MC.scenario([(10.0 + t, 20.0) for t in range(T)], [t == 6 for t in range(T)])
        return x, MR.scenario_run(x, 2.0, 10, MC.SCALARS)
    c = MC.CASES[0 if scene in ("gap", "empty") else scene]
    x = {k: np.ascontiguousarray(v[:, list(LANES)]) for k, v in MC.make(c).items()}
    if scene == "gap":
        x["best_row"][list(GAP_FRAMES), GAP_LANE] = -1
    if scene == "empty":
        x = {k: np.ascontiguousarray(v[:, EMPTY:EMPTY + 1]) for k, v in x.items()}
    return x, MR.identity(M=c.M, appearance=c.appearance, optimal=c.optimal, **kw, **x)


@functools.lru_cache(maxsize=None)
def make(name):
    """{lane_id, track_len [T', B, N] int32, best_row [T', B] int32, box [T', B, N, 4] float32} of the case: what the append is fed,
    the frames of all its passes; made once, never written to."""
    c = CASES[name]
    x, run = identity_run(c.scene)
    n = sum(c.passes)
    out = dict(lane_id=run.lane_id[:n].astype(np.int32), track_len=run.track_len[:n].astype(np.int32),
               best_row=x["best_row"][:n].astype(np.int32), box=x["box"][:n].astype(np.float32))
    for a in out.values():
        a.setflags(write=False)
    return out


def passes(name):
    """The case's frames as its passes: [(first, last + 1)]."""
    at, out = 0, []
    for n in CASES[name].passes:
        out.append((at, at + n))
        at += n
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(the inputs, the reference's log after all passes, the reference's solve of it): made once, never written to."""
    c = CASES[name]
    x = make(name)
    log = R.new_log(x["best_row"].shape[1], c.L, c.N)
    for lo, hi in passes(name):
        log = R.append(log, *[x[k][lo:hi] for k in INPUTS])
    for a in log.values():
        a.setflags(write=False)
    return x, log, R.smooth(log, c.lag, c.C, Q, R_MEAS, V0_VAR)


# ------------------------------------------------------------------------------------------------ the kernels on caller buffers (GPU)
HW = MC.HW
PARITY_NOTE = ("per case of tests/test_tracklog_kernel.py (and, under 'stream', of tests/test_tracklog_stream.py): the bars of filt and "
               "smooth -- four times the measured error of the fp32 restatement of the header against float64 "
               "(tests/tracklog_ref.py) --, the kernel's own error against float64, and what the case holds; the integer outputs, "
               "size and the log's bytes are compared exactly")


def record(section, case, **figures):
    """One case's figures into tracklog_parity.json under SQAIR_PARITY_DIR."""
    import torch
    from sqair_amd import _capi
    from tests.kernel_unit import merge_parity

    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data.setdefault(section, {})[case] = figures
    merge_parity("tracklog_parity.json", lambda: {"note": PARITY_NOTE, "cases": {}, "stream": {}}, update)


def handle(N, wide=False, nw=6):
    """A handle of N object slots, kept for the session: the append reads the handle's N."""
    from tests.abi_host import LANE_LIBS, kept_handle
    return kept_handle(("tracklog", N, wide, nw), LANE_LIBS["wide" if wide else "product"], HW, k_particles=2, n_steps_per_image=N, n_what=nw)


def to_device(arrays):
    import torch
    return {n: torch.from_numpy(np.array(v)).cuda() for n, v in arrays.items()}


def log_struct(d, L):
    from sqair_amd import _capi
    return _capi.SqairLaneTrackLog(L=L, **{n: d[n].data_ptr() for n in _capi.TRACKLOG_FIELDS})


def run_append(lib, h, x, d, L, stream=None):
    """One launch of k_lane_tracklog on the device frames ``x`` (of INPUTS), continuing the device log ``d`` in place."""
    import ctypes as C
    import torch
    T, B = x["best_row"].shape
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = lib.sqair_lane_tracklog_test(h, *[x[k].data_ptr() for k in INPUTS], T, B, C.byref(log_struct(d, L)), s)
    assert rc == 0, lib.sqair_last_error(h)


def solve_buffers(lib, lag, B, C_, N):
    """(the solve's outputs, filled with -7 so that every word must be written, the scratch with any content)."""
    import torch
    from sqair_amd import _capi
    out = {k: torch.full(shp, -7, dtype=getattr(torch, _capi.field_dtype("SqairTrackLogOut", k)), device="cuda")
           for k, shp in _capi.tracklog_out_shapes(lag, B, C_).items()}
    work = torch.full((B * lib.sqair_lane_tracklog_work_bytes(lag, C_, N) // 4,), 12345, dtype=torch.int32, device="cuda")
    return out, work


def run_smooth(lib, h, d, L, lag, C_, N, out, work, scalars=(Q, R_MEAS, V0_VAR), stream=None):
    """One launch of k_lane_tracklog_smooth on the device log ``d`` into ``out``."""
    import ctypes as C
    import torch
    from sqair_amd import _capi
    B = d["count"].shape[0]
    o = _capi.SqairTrackLogOut(**{n: t.data_ptr() for n, t in out.items()})
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = lib.sqair_lane_tracklog_smooth(h, C.byref(log_struct(d, L)), lag, C_, N, B, *scalars, C.byref(o), work.data_ptr(), s)
    assert rc == 0, lib.sqair_last_error(h)


def motion_kernel(name):
    """sqair_lane_identity_motion_test on the case's scene with motion_cases' scalars: {lane_id, track_len, velocity} (host) -- what
    the solve's forward filter is compared with as bits."""
    import ctypes as C
    import torch
    from sqair_amd import _capi
    from tests import identity_ref as IR
    c = CASES[name]
    x = identity_run(c.scene)[0]
    T_, B, N = x["presence"].shape
    scenario = c.scene in ("dropout", "once")
    mc = MC.CASES[0 if c.scene in ("gap", "empty") else c.scene] if not scenario else None
    M, nw, app = (1, 1, False) if scenario else (mc.M, mc.nw, mc.appearance)
    reid, age = (2.0, 10) if scenario else (MC.REID_DIST, MC.MAX_AGE)
    lib, h = handle(N, c.wide, nw)
    assert lib.sqair_set_lane_match(h, 0, 0, 0) == 0
    mem = {k: torch.from_numpy(v).cuda() for k, v in IR.fresh_memory(B, M, nw, app).items() if v is not None}
    kf = torch.zeros((B, M, 2, 5), dtype=torch.float32, device="cuda")
    o = {n: torch.full((T_, B, N), -7, dtype=torch.int32, device="cuda") for n in _capi.IDENT_FIELDS}
    vel = torch.full((T_, B, N, 2), -7.0, device="cuda")
    d = to_device(x)
    idt = _capi.SqairLaneIdentity(iou_min=MC.IOU_MIN, reid_dist=reid, reid_what=float("inf"), M=M, max_age=age,
                                  **{n: t.data_ptr() for n, t in mem.items()}, **{n: o[n].data_ptr() for n in _capi.IDENT_FIELDS})
    mo = _capi.SqairLaneMotion(q=MC.Q, r=MC.R_MEAS, v0_var=MC.V0_VAR, gate=MC.GATE, trk_kf=kf.data_ptr(), velocity=vel.data_ptr(), nis=None)
    rc = lib.sqair_lane_identity_motion_test(h, *[d[k].data_ptr() for k in ("box", "presence", "obj_id", "what", "best_row")], T_, B,
                                             C.byref(idt), C.byref(mo), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return dict(lane_id=o["lane_id"].cpu().numpy(), track_len=o["track_len"].cpu().numpy(), velocity=vel.cpu().numpy())
