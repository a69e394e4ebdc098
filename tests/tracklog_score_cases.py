"""The inputs of the track log scoring tests (tests/test_tracklog_score_ref.py on the CPU, tests/test_tracklog_score_kernel.py on the
GPU): a log, the window and the columns it is solved with, and the truth of the window's frames -- at most 8 lanes of 16 frames.

Cases a, d, e, f, g, h and j are the track log's own (tests/tracklog_cases.py: ``reference``), with truth added:
  h, j   scenes with known centres (motion_cases' ``moving_dropout``; the empty lane): the truth is the TRUE box;
  a, d, e, f, g   random scenes: the truth of slot g is the reference solve's smoothed box of a chosen column, moved by a fixed offset,
         wherever that column is seen or in a gap.  Every third column is given to no truth (false positives), the last slot holds a
         truth far outside the field that nobody tracks (misses), and slot 0 has a hole in truth_present in the middle of the window.
New cases:
  w   case f's log with G = 16 against C = 64, on the wide library;
  v   case a's log with holes in truth_valid;
  x   a log made by hand, four lanes of N = 2 slots, every track stationary -- the filter and the smoother then return the measured
      centre exactly, so the IoUs are the boxes' own --:
        lane 0  two truths over two tracks with match_cases' table [[0.60, 0.54], [0.54, 0.08]]: greedy matches one pair a frame, optimal two;
        lane 1  a truth followed by track 3 and then by track 5 (idsw 1; the window's identity assignment gives the tail to nobody);
        lane 2  five frames logged under a window of twelve: the window reaches before the lane's first record;
        lane 3  a moving track with a two-frame gap, a non-finite frame with valid truth (frames_invalid) and holes in truth_valid.

CONDITION, not a measurement: the offsets are chosen so that no candidate IoU lies within 1e-5 of iou_min and no two competing
candidates lie within 1e-5 of each other (``score_ref.fragile_from``'s rule per view, ``tracklog_score_ref.fragile``);
tests/test_tracklog_score_ref.py asserts that NO (lane, view) of any case is fragile, so nothing is ever left out of an exact
comparison.  If a case trips it, the offset moves, not the rule."""
import collections
import functools

import numpy as np

from tests import motion_cases as MC
from tests import tracklog_cases as TC
from tests import tracklog_ref as R
from tests import tracklog_score_ref as SR

IOU_MIN = 0.5
Case = collections.namedtuple("Case", "name base G")
CASES = collections.OrderedDict((c.name, c) for c in (
    Case("a", "a", 4), Case("d", "d", 3), Case("e", "e", 2), Case("f", "f", 6), Case("g", "g", 4), Case("h", "h", 2), Case("j", "j", 2),
    Case("w", "f", 16), Case("v", "a", 4), Case("x", None, 2)))
# the offset (y, x, h, w) of truth slot g from the smoothed box it follows: OFFSET * (1 + OFFSET_STEP * g)
OFFSET = np.array([0.6, -0.4, 0.5, -0.3])
OFFSET_STEP = 0.17
FAR = (-40.0, -40.0, 8.0, 8.0)           # the truth nobody tracks: outside the field the boxes live in (motion_cases: LO = -10)
X_SHAPE = dict(N=2, C=4, L=16, lag=12)

Inputs = collections.namedtuple("Inputs", "N C L lag wide log solve truth")


def shape(name):
    """(N, C, L, lag, wide) of a case."""
    c = CASES[name]
    if c.base is None:
        return X_SHAPE["N"], X_SHAPE["C"], X_SHAPE["L"], X_SHAPE["lag"], False
    t = TC.CASES[c.base]
    return t.N, t.C, t.L, t.lag, t.wide


# ---- the hand-made log ------------------------------------------------------------------------------------------------------------
def _lane_log(frames, N, L):
    """A log of ONE lane from ``frames``: per frame None (a non-finite frame) or a list of (lane_id, track_len, (y, x, h, w)) by slot."""
    T = len(frames)
    lane_id, track_len = -np.ones((T, 1, N), np.int32), -np.ones((T, 1, N), np.int32)
    best_row, box = np.zeros((T, 1), np.int32), np.zeros((T, 1, N, 4), np.float32)
    for t, fr in enumerate(frames):
        if fr is None:
            best_row[t, 0] = -1
            continue
        for j, (i, n, bx) in enumerate(fr):
            lane_id[t, 0, j], track_len[t, 0, j], box[t, 0, j] = i, n, bx
    return R.append(R.new_log(1, L, N), lane_id, track_len, best_row, box)


def _row(x, w=20.0):
    """match_cases' boxes: height 20 at y = 0, only x and the width differ."""
    return (0.0, float(x), 20.0, float(w))


@functools.lru_cache(maxsize=None)
def _hand():
    """(log of the four lanes, truth) of case x."""
    N, L, lag, G = X_SHAPE["N"], X_SHAPE["L"], X_SHAPE["lag"], CASES["x"].G
    tb, tp, tv = np.zeros((lag, 4, G, 4), np.float32), np.zeros((lag, 4, G), np.int32), np.ones((lag, 4), np.int32)
    # lane 0: widths 20 at x = 4 (track 1), 10 (truth 0), 15 (track 0), 21 (truth 1): 15/25, 14/26, 14/26, 3/37
    l0 = _lane_log([[(0, t + 1, _row(15)), (1, t + 1, _row(4))] for t in range(lag)], N, L)
    tb[:, 0, 0], tb[:, 0, 1], tp[:, 0] = _row(10), _row(21), 1
    # lane 1: one object at the same place, lane_id 3 for six frames, then 5
    l1 = _lane_log([[(3 if t < 6 else 5, (t if t < 6 else t - 6) + 1, (10.0, 12.0, 10.0, 10.0))] for t in range(lag)], N, L)
    tb[:, 1, 0], tp[:, 1, 0] = (10.5, 11.5, 10.0, 10.0), 1
    # lane 2: five frames logged: window frames 0..6 have no record (their truth, valid, must change nothing)
    l2 = _lane_log([[(0, t + 1, (20.0, 20.0, 12.0, 12.0))] for t in range(5)], N, L)
    tb[:, 2, 1], tp[:, 2, 1] = (20.5, 20.0, 12.0, 12.0), 1
    # lane 3: a track moving 2 px a frame along x, unseen in frames 4 and 5; frame 8 non-finite; no truth in frames 1 and 9
    fr = [[(7, t + 1, (5.0, 4.0 + 2.0 * t, 10.0, 10.0))] for t in range(lag)]
    fr[4], fr[5], fr[8] = [], [], None
    l3 = _lane_log(fr, N, L)
    for t in range(lag):
        tb[t, 3, 0], tp[t, 3, 0] = (5.25, 4.0 + 2.0 * t, 10.0, 10.0), 1
    tv[[1, 9], 3] = 0
    log = {k: np.concatenate([l[k] for l in (l0, l1, l2, l3)]) for k in R.FIELDS}
    return log, dict(truth_box=tb, truth_present=tp, truth_valid=tv)


# ---- truth for the track log's own cases --------------------------------------------------------------------------------------------
def _true_boxes(name, lag, G):
    """Cases h and j: the true box of the one object in slot 0 (h), nothing (j)."""
    tb, tp = np.zeros((lag, 1, G, 4), np.float32), np.zeros((lag, 1, G), np.int32)
    if name == "h":
        true = MC.moving_dropout()[1]
        for f in range(lag):
            tb[f, 0, 0], tp[f, 0, 0] = (true[f, 0] - 5.0, true[f, 1] - 5.0, 10.0, 10.0), 1
    else:
        tb[:, 0, 1], tp[:, 0, 1] = FAR, 1
    return tb, tp


def _followed_boxes(solve, lag, G):
    """The random scenes: slot g < G - 1 follows the g-th column that is not given up (every third is), the last slot is FAR."""
    B, C = solve.track_id.shape
    tb, tp = np.zeros((lag, B, G, 4), np.float32), np.zeros((lag, B, G), np.int32)
    centre = solve.smooth32[..., 0]                                             # [lag, B, C, 2]
    box = np.concatenate([centre - 0.5 * solve.size, solve.size], -1).astype(np.float64)
    for b in range(B):
        owned = [c for c in range(C) if solve.track_id[b, c] >= 0 and c % 3 != 2][:G - 1]
        for g, c in enumerate(owned):
            on = (solve.state[:, b, c] == R.SEEN) | (solve.state[:, b, c] == R.GAP)
            tb[on, b, g] = (box[on, b, c] + OFFSET * (1.0 + OFFSET_STEP * g)).astype(np.float32)
            tp[on, b, g] = 1
        tp[lag // 2, b, 0] = 0                                                  # the hole
        tb[:, b, G - 1], tp[:, b, G - 1] = FAR, 1
    return tb, tp


@functools.lru_cache(maxsize=None)
def inputs(name):
    """``Inputs`` of a case: the shape, the log {name: array}, the reference's solve of it (tracklog_ref.Smooth) and the truth in window
    order {truth_box, truth_present, truth_valid}.  Made once, never written to."""
    c = CASES[name]
    N, C, L, lag, wide = shape(name)
    if c.base is None:
        log, truth = _hand()
        solve = R.smooth(log, lag, C, TC.Q, TC.R_MEAS, TC.V0_VAR)
    else:
        _, log, solve = TC.reference(c.base)
        B = solve.track_id.shape[0]
        tb, tp = _true_boxes(name, lag, c.G) if name in ("h", "j") else _followed_boxes(solve, lag, c.G)
        tv = np.ones((lag, B), np.int32)
        if name == "v":
            tv[np.arange(lag)[:, None] % 3 == np.arange(B)[None, :] % 3] = 0
            tv[:, 5] = 0
        truth = dict(truth_box=tb, truth_present=tp, truth_valid=tv)
    for a in truth.values():
        a.setflags(write=False)
    return Inputs(N, C, L, lag, wide, log, solve, truth)


def table_of(solve):
    """The solve's outputs the scorer reads, {name: array}: the fp32 restatement's words stand for filt and smooth."""
    return dict(track_id=solve.track_id, frame_index=solve.frame_index, state=solve.state, size=solve.size, filt=solve.filt32,
                smooth=solve.smooth32)


@functools.lru_cache(maxsize=None)
def reference(name, match="greedy"):
    """The reference's score of a case on the reference's own solve: made once, never written to."""
    x = inputs(name)
    return SR.score(table_of(x.solve), x.log["log_valid"], x.truth, IOU_MIN, match)


# ------------------------------------------------------------------------------------------------ the kernel on caller buffers (GPU)
PARITY_NOTE = ("per case of tests/test_tracklog_score_kernel.py and per matching: the worst fp32 error of a term of each sum -- the fp32 "
               "restatement of the header against float64 (tests/tracklog_score_ref.py); a sum's bar is four times that times its "
               "number of terms --, the kernel's own worst error of each sum against float64 and the bar it was held to, and what the "
               "case holds; every integer output is compared exactly")


def record(section, case, **figures):
    """One case's figures into tracklog_score_parity.json under SQAIR_PARITY_DIR."""
    import torch
    from sqair_amd import _capi
    from tests.kernel_unit import merge_parity

    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data.setdefault(section, {})[case] = figures
    merge_parity("tracklog_score_parity.json", lambda: {"note": PARITY_NOTE, "cases": {}, "stream": {}}, update)


def score_buffers(lag, B, G):
    """The scorer's outputs, filled with -7 so that every word must be written."""
    import torch
    from sqair_amd import _capi
    return {k: torch.full(shp, -7, dtype=getattr(torch, _capi.field_dtype("SqairTrackLogScore", k)), device="cuda")
            for k, shp in _capi.tracklog_score_shapes(lag, B, G).items()}


def run_score(lib, h, d, L, table, truth, out, lag, C_, G, match, iou_min=IOU_MIN, stream=None):
    """One launch of k_lane_tracklog_score: device log ``d``, the solve's device outputs ``table``, device ``truth``, into ``out``."""
    import ctypes as C
    import torch
    from sqair_amd import _capi
    B = d["count"].shape[0]
    tab = _capi.SqairTrackLogOut(**{n: table[n].data_ptr() for n in _capi.TRACKLOG_SCORE_TABLE})
    tr = _capi.SqairTrackLogTruth(G=G, **{n: truth[n].data_ptr() for n in _capi.TRACKLOG_TRUTH_FIELDS})
    sc = _capi.SqairTrackLogScore(iou_min=iou_min, **{n: t.data_ptr() for n, t in out.items()})
    s = C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)
    rc = lib.sqair_lane_tracklog_score(h, C.byref(TC.log_struct(d, L)), C.byref(tab), C.byref(tr), C.byref(sc), lag, C_, B, match, s)
    assert rc == 0, lib.sqair_last_error(h)
