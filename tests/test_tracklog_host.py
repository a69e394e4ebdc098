"""No GPU: the C-ABI of the track log (include/sqair_hip.h: sqair_set_tracklog, sqair_lane_tracklog_test, sqair_lane_tracklog_smooth,
sqair_lane_tracklog_work_bytes) -- exported and declared, the binding mirrors the header's structs, the track log paragraph carries
the semantics, every refusal of the three entries is made before any HIP call (dummy device pointers are enough) and leaves the
handle as it was, the log goes off with the identity (and so with the estimate and the state) -- and the argument errors of
SqairStream(tracklog=...) and mot_rows' companion ``track_log``."""
import ctypes as C
import functools
import os

import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, c_layout, dummy, err as _err, estimate, fields as header_fields, fwd_args, handle,
                            paragraph, phrases, prototype, set_state as _state, stated_once, constant)

INF = float("inf")
N = 3
_est = functools.partial(estimate, fields=("box", "presence", "obj_id", "map_count", "what"))


def _ident(M=6, without=()):
    idt = dummy(_capi.SqairLaneIdentity, 0x5000, _capi.IDENT_MEMORY, iou_min=0.3, reid_dist=4.0, reid_what=INF, M=M, max_age=10)
    for i, n in enumerate(_capi.IDENT_FIELDS):
        if n not in without:
            setattr(idt, n, 0x7000 + 0x100 * i)
    return idt


def _log(L=8, without=()):
    return dummy(_capi.SqairLaneTrackLog, 0xa000, _capi.TRACKLOG_FIELDS, without, L=L)


def _out(without=()):
    return dummy(_capi.SqairTrackLogOut, 0xb000, _capi.TRACKLOG_OUT_FIELDS, without)


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged(tmp_path):
    names = ("sqair_set_tracklog", "sqair_lane_tracklog_test", "sqair_lane_tracklog_smooth", "sqair_lane_tracklog_work_bytes")
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert all(hasattr(lib, n) for n in names) and lib.sqair_abi_version() == 2
    assert all(n in _capi.EXPORTED_SYMBOLS for n in names) and _capi.ABI_VERSION == 2
    assert prototype("sqair_set_tracklog") == "int sqair_set_tracklog(SqairHandle* h, const SqairLaneTrackLog* log, int T, int B)"
    assert prototype("sqair_lane_tracklog_test") == (
        "int sqair_lane_tracklog_test(SqairHandle* h, const int32_t* lane_id, const int32_t* track_len, const int32_t* best_row, "
        "const float* box, int T, int B, const SqairLaneTrackLog* log, void* stream)")
    assert prototype("sqair_lane_tracklog_smooth") == (
        "int sqair_lane_tracklog_smooth(SqairHandle* h, const SqairLaneTrackLog* log, int lag, int C, int N, int B, float q, float r, "
        "float v0_var, const SqairTrackLogOut* out, void* work, void* stream)")
    assert prototype("sqair_lane_tracklog_work_bytes") == "int64_t sqair_lane_tracklog_work_bytes(int lag, int C, int N)"
    fields = header_fields("SqairLaneTrackLog")
    assert fields == [("int32_t", "L"), ("int64_t*", "count"), ("int32_t*", "log_valid"), ("int32_t*", "log_id"), ("int32_t*", "log_len"),
                      ("float*", "log_box")]
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairLaneTrackLog._fields_] == ["L"] + list(_capi.TRACKLOG_FIELDS)
    out = header_fields("SqairTrackLogOut")
    assert out == [("int32_t*", "track_id"), ("int32_t*", "n_tracks"), ("int32_t*", "len0"), ("int64_t*", "frame_index"),
                   ("int32_t*", "state"), ("float*", "size"), ("float*", "filt"), ("float*", "smooth")]
    assert [n for _, n in out] == [n for n, _ in _capi.SqairTrackLogOut._fields_] == list(_capi.TRACKLOG_OUT_FIELDS)
    # the compiler's layout is the binding's
    lay = c_layout(tmp_path, {"SqairLaneTrackLog": ["L", "count", "log_box"], "SqairTrackLogOut": ["track_id", "frame_index", "smooth"]})
    assert lay["SqairLaneTrackLog"] == (C.sizeof(_capi.SqairLaneTrackLog), [0, _capi.SqairLaneTrackLog.count.offset,
                                                                             _capi.SqairLaneTrackLog.log_box.offset]) == (48, [0, 8, 40])
    assert lay["SqairTrackLogOut"] == (C.sizeof(_capi.SqairTrackLogOut), [0, 24, 56]) == (64, [0, 24, 56])
    assert constant("SQAIR_TRACKLOG_MAX_FRAMES") == 4096 == _capi.TRACKLOG_MAX_FRAMES
    assert constant("SQAIR_TRACKLOG_MAX_TRACKS") == 64 == _capi.TRACKLOG_MAX_TRACKS
    assert _capi.tracklog_shapes(2, 8, 3) == dict(count=(2,), log_valid=(2, 8), log_id=(2, 8, 3), log_len=(2, 8, 3), log_box=(2, 8, 3, 4))
    assert _capi.tracklog_out_shapes(5, 2, 4) == dict(track_id=(2, 4), n_tracks=(2,), len0=(2, 4), frame_index=(5, 2), state=(5, 2, 4),
                                                      size=(5, 2, 4, 2), filt=(5, 2, 4, 2, 5), smooth=(5, 2, 4, 2, 5))
    assert _capi.field_dtype("SqairLaneTrackLog", "count") == "int64" and _capi.field_dtype("SqairTrackLogOut", "frame_index") == "int64"
    assert _capi.TRACKLOG_OUT_INT_FIELDS == ("track_id", "n_tracks", "len0", "state")


def test_the_header_states_the_semantics_once():
    doc = paragraph("the track log: trajectories per lane_id", "#define SQAIR_TRACKLOG_MAX_FRAMES")
    phrases(doc, ("the track log paragraph", "k_lane_tracklog", "directly after the identity's node", "BEFORE k_lane_score",
                  "BEFORE the SMC resampler", "exactly one kernel node more", "nothing is launched", "unchanged bit for bit",
                  "Training passes", "eager pre-pass without effects", "never run it",
                  "reads only the identity's own output buffers lane_id and track_len and the estimate's box and best_row",
                  "L in 1..4096 records", "count [B] int64", "invalid ones included", "the caller starts it at 0",
                  "(count[b] + t) mod L", "count[b] += T", "log_valid [B,L]", "best_row[t,b] == -1", "log_id [B,L,N]",
                  "-1 where slot j is absent", "log_len [B,L,N]", "log_box [B,L,N,4]", "copied as they are",
                  "Every word of the record is written", "stale words are never read", "wrap-around needs no case of its own",
                  "a replayed graph leaves the bytes of eager calls",
                  "two passes of five and seven frames leave the bytes of one pass of twelve",
                  "sqair_lane_tracklog_smooth", "stand-alone capturable call", "k_lane_tracklog_smooth", "one workgroup per lane",
                  "It registers nothing", "it writes only its outputs and `work`", "may interleave with passes", "C in 1..64",
                  "1. Window", "g = count[b] - lag + f", "g mod L", "frame_index = -1", "A frame COUNTS",
                  "2. Columns", "n_tracks[b] is their number", "The C largest are kept", "listed ascending", "padded with -1",
                  "the smallest such j", "len0[b,c]", "born inside the window",
                  "3. Forward filter", "one thread per (column, axis", "the motion paragraph's P and U", "z = fmaf(0.5, size, origin)",
                  "whatever len0 is", "(z, 0, r, 0, v0_var)", "state 1, seen", "state 2, a gap", "does not step", "(state 3)",
                  "Outside the span the state is 0",
                  "4. Backward pass (Rauch-Tung-Striebel)", "in descending order", "exactly one P apart",
                  "At f1 the smoothed state is the filtered one",
                  "pm = p + v; am = ((a + 2 b) + c) + q/4; bm = (b + c) + q/2; cm = c + q",
                  "det = fmaf(am, cm, -(bm bm)); m00 = a + b; m10 = b + c",
                  "g00 = fmaf(m00, cm, -(b bm)) / det; g01 = fmaf(b, am, -(m00 bm)) / det",
                  "g10 = fmaf(m10, cm, -(c bm)) / det; g11 = fmaf(c, am, -(m10 bm)) / det",
                  "G = P F^T (P-)^-1, F = [[1,1],[0,1]]",
                  "dp = ps+ - pm; dv = vs+ - v; da = as+ - am; db = bs+ - bm; dc = cs+ - cm",
                  "ps = fmaf(g01, dv, fmaf(g00, dp, p)); vs = fmaf(g11, dv, fmaf(g10, dp, v))",
                  "e00 = fmaf(g01, db, g00 da); e01 = fmaf(g01, dc, g00 db); e10 = fmaf(g11, db, g10 da); e11 = fmaf(g11, dc, g10 db)",
                  "as = fmaf(e01, g01, fmaf(e00, g00, a)); bs = fmaf(e01, g11, fmaf(e00, g10, b)); cs = fmaf(e11, g11, fmaf(e10, g10, c))",
                  "P_s = P + G (P_s+ - P-) G^T", "only that is stored",
                  "5. Outputs", "state [lag,B,C] int32", "filt and smooth [lag,B,C,2,5]", "0 where the state is 0 or 3",
                  "size [lag,B,C,2]", "the last seen ones at state 2", "sizes are not filtered", "All arithmetic is fp32",
                  "every sum in one fixed order", "no decision depends on a threshold", "the same bits come out of every replay",
                  "has the bits of the motion's velocity",
                  "B * sqair_lane_tracklog_work_bytes(lag, C, N) bytes", "neither fits LDS",
                  "NULL log: off", "refused", "no identity set", "an identity without track_len bound", "a T other than the estimate's",
                  "a B other than the state's", "L outside 1..4096", "a NULL count, log_valid, log_id, log_len or log_box",
                  "switches the log off", "registering an identity without track_len",
                  "Out of scope", "filtering h, w", "lane tracks and lane forecasts", "scoring the log against truth", "training passes",
                  "identities across lanes"))
    stated_once("the track log: trajectories per lane_id")
    solve = paragraph("The solve (points 1 to 5)", "typedef struct SqairTrackLogOut")
    phrases(solve, ("Every output is required", "Refused", "a NULL log, out or work", "lag outside 1..L", "C outside 1..64",
                    "N outside 1..16", "B < 1", "not finite and positive", "what sqair_set_tracklog refuses for log"))
    for name in ("DESIGN.md", "README.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "sqair_set_tracklog" in text and "sqair_lane_tracklog_smooth" in text, name


@pytest.mark.parametrize("path", LIBS)
def test_set_tracklog_refusals_before_any_hip_call_leave_the_handle_unchanged(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        B, T = 4, 2
        on = lambda g=None, t=T, b=B: lib.sqair_set_tracklog(h, C.byref(g or _log()), t, b)
        assert lib.sqair_set_tracklog(None, C.byref(_log()), T, B) == -1
        assert on() == -1 and "needs an identity (sqair_set_identity)" in _err(lib, h)          # no state, no estimate, no identity
        _state(lib, h, B)
        assert on() == -1 and "needs an identity" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
        assert on() == -1 and "needs an identity" in _err(lib, h)                               # an estimate, no identity
        assert lib.sqair_set_identity(h, C.byref(_ident(without=("track_len",))), T, B) == 0
        assert on() == -1 and "must bind track_len" in _err(lib, h)                             # an identity without track_len
        assert lib.sqair_set_identity(h, C.byref(_ident()), T, B) == 0
        assert on() == 0
        for t in (1, 3, 0):
            assert on(t=t) == -1 and "T = {}".format(t) in _err(lib, h) and "T = 2" in _err(lib, h)
        assert on(b=B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        for L in (0, -1, 4097):
            assert on(_log(L=L)) == -1 and "L = {} must lie in 1..4096".format(L) in _err(lib, h)
        for missing in _capi.TRACKLOG_FIELDS:
            assert on(_log(without=(missing,))) == -1 and "count, log_valid, log_id, log_len and log_box must not be NULL" in _err(lib, h)
        for L in (1, 4096):
            assert on(_log(L=L)) == 0
        assert lib.sqair_set_tracklog(h, None, 0, 0) == 0 and on() == 0                         # NULL: off; and on again
        assert lib.sqair_set_identity(h, C.byref(_ident()), T, B) == 0                          # the identity re-registered: it stays
        assert lib.sqair_set_tracklog(h, None, 0, 0) == 0
        # a pass of another T is refused for the estimate's T with or without a log; training never runs it
        assert on() == 0
        for t in (1, 3):
            assert lib.sqair_forward(*fwd_args(h, B, T=t)) == -1 and "T = 2" in _err(lib, h)
        assert lib.sqair_forward_train(*fwd_args(h, B, T=2)) == -1 and "carried state" in _err(lib, h)


def test_the_identity_going_off_takes_the_log_with_it():
    """The log can only be set while an identity with track_len is: after anything that switches the identity off a NULL-free
    sqair_set_tracklog is refused until the identity is set again -- and setting the identity again does not bring an old log back."""
    with handle(k_particles=2, n_steps_per_image=N) as (lib, h):
        B = 4
        ident = lambda T=2, b=B, **kw: lib.sqair_set_identity(h, C.byref(_ident(**kw)), T, b)
        on = lambda T=2, b=B: lib.sqair_set_tracklog(h, C.byref(_log()), T, b)
        refused = lambda T=2, b=B: on(T, b) == -1 and "needs an identity" in _err(lib, h)
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and ident() == 0 and on() == 0
        assert lib.sqair_set_identity(h, None, 0, 0) == 0 and refused()                         # the identity off
        assert ident() == 0 and on() == 0
        assert ident(without=("track_len",)) == 0                                               # ... or re-registered without track_len
        assert on() == -1 and "must bind track_len" in _err(lib, h)
        assert ident() == 0 and on() == 0
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0 and refused()                         # the estimate off
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and refused() and ident() == 0 and on() == 0
        assert lib.sqair_set_estimate(h, C.byref(_est(without=("box",))), 2, B) == 0            # a field of the identity's goes
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and refused() and ident() == 0 and on() == 0
        assert lib.sqair_set_estimate(h, C.byref(_est()), 3, B) == 0 and refused(3)             # another T
        assert ident(3) == 0 and on(2) == -1 and on(3) == 0
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0 and refused(3)               # the state off
        _state(lib, h, B)
        assert refused(3)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and ident() == 0 and on() == 0
        _state(lib, h, B + 1)                                                                   # another B
        assert refused(2, B + 1)
        # beside the motion: each goes its own way, both go with the identity
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B + 1) == 0 and ident(2, B + 1) == 0 and on(2, B + 1) == 0
        mo = dummy(_capi.SqairLaneMotion, 0x9000, ("trk_kf", "velocity"), q=0.25, r=1.0, v0_var=16.0, gate=3.0)
        assert lib.sqair_set_motion(h, C.byref(mo), 2, B + 1) == 0 and lib.sqair_set_motion(h, None, 0, 0) == 0 and on(2, B + 1) == 0
        assert lib.sqair_set_tracklog(h, None, 0, 0) == 0 and lib.sqair_set_motion(h, C.byref(mo), 2, B + 1) == 0


@pytest.mark.parametrize("path", LIBS)
def test_kernel_entry_point_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        good = dict(lane_id=DUMMY, track_len=DUMMY, best_row=DUMMY, box=DUMMY, T=1, B=3)
        order = ("lane_id", "track_len", "best_row", "box", "T", "B")
        call = lambda g, **kw: lib.sqair_lane_tracklog_test(h, *[dict(good, **kw)[k] for k in order],
                                                            C.byref(g) if g is not None else None, DUMMY)
        assert lib.sqair_lane_tracklog_test(None, *[good[k] for k in order], C.byref(_log()), DUMMY) == -1
        for kw in (dict(lane_id=None), dict(track_len=None), dict(best_row=None), dict(box=None), dict(T=0), dict(T=65536), dict(B=0)):
            assert call(_log(), **kw) == -1 and "sqair_lane_tracklog_test" in _err(lib, h), kw
        assert call(None) == -1
        for L in (0, 4097):
            assert call(_log(L=L)) == -1 and "must lie in 1..4096" in _err(lib, h)
        for missing in _capi.TRACKLOG_FIELDS:
            assert call(_log(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h)


@pytest.mark.parametrize("path", LIBS)
def test_the_solves_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        good = dict(log=_log(L=8), lag=8, C=4, N=3, B=2, q=0.25, r=1.0, v0_var=16.0, out=_out(), work=DUMMY)
        order = ("lag", "C", "N", "B", "q", "r", "v0_var")

        def call(**kw):
            a = dict(good, **kw)
            ref = lambda v: C.byref(v) if v is not None else None
            return lib.sqair_lane_tracklog_smooth(h, ref(a["log"]), *[a[k] for k in order], ref(a["out"]), a["work"], DUMMY)
        assert lib.sqair_lane_tracklog_smooth(None, C.byref(good["log"]), *[good[k] for k in order], C.byref(good["out"]), DUMMY, DUMMY) == -1
        for kw in (dict(log=None), dict(out=None), dict(work=None)):
            assert call(**kw) == -1 and "log, out and work must not be NULL" in _err(lib, h), kw
        for lag in (0, -1, 9, 4097):
            assert call(lag=lag) == -1 and "lag" in _err(lib, h) and "1..L" in _err(lib, h), lag
        for Cn in (0, 65):
            assert call(C=Cn) == -1 and "C must lie in 1..64" in _err(lib, h)
        for n in (0, 17):
            assert call(N=n) == -1 and "N must lie in 1..16" in _err(lib, h)
        assert call(B=0) == -1 and "B = 0 must be >= 1" in _err(lib, h)
        for name in ("q", "r", "v0_var"):
            for bad in (0.0, -1.0, INF, -INF, float("nan")):
                assert call(**{name: bad}) == -1 and name + " must be finite and > 0" in _err(lib, h), (name, bad)
        for missing in _capi.TRACKLOG_OUT_FIELDS:
            assert call(out=_out(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h), missing
        for L in (0, 4097):                                                             # what sqair_set_tracklog refuses for the log
            assert call(log=_log(L=L)) == -1 and "must lie in 1..4096" in _err(lib, h)
        for missing in _capi.TRACKLOG_FIELDS:
            assert call(log=_log(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h)
        # the scratch query: per lane, one int32 per (frame, column); 0 for what the solve refuses
        wb = lib.sqair_lane_tracklog_work_bytes
        assert wb(8, 4, 3) == 8 * 4 * 4 and wb(4096, 64, 16) == 4096 * 64 * 4 and wb(1, 1, 1) == 4
        assert wb(0, 4, 3) == wb(4097, 4, 3) == wb(8, 0, 3) == wb(8, 65, 3) == wb(8, 4, 0) == wb(8, 4, 17) == 0


def test_stream_argument_errors():
    """The log's arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    for kw in (dict(), dict(estimate=True)):
        with pytest.raises(ValueError, match=r"^SqairStream: tracklog is for a stream with identity=True"):
            SqairStream(Core(), 2, tracklog=8, **kw)
    for bad in (0, -1, 4097, 8.0, True, "8"):
        with pytest.raises(ValueError, match=r"^SqairStream: tracklog must be an integer in \[1, 4096\]"):
            SqairStream(Core(), 2, estimate=True, identity=True, tracklog=bad)
    for bad in (0, 65, 2.0, None):
        with pytest.raises(ValueError, match=r"^SqairStream: tracklog_tracks must be an integer in \[1, 64\]"):
            SqairStream(Core(), 2, estimate=True, identity=True, tracklog=8, tracklog_tracks=bad)
    # without a log the read-out says which switch is missing
    from sqair_amd.lane import LaneAnswers
    la = LaneAnswers("SqairStream", True, 0.5, False, False, 0.5, False, 0.5, None, True, 0.3, None, 10, 4.0, INF, True, "row")
    with pytest.raises(ValueError, match=r"^SqairStream.track_log: the stream keeps no track log .*tracklog=L"):
        la.track_log()
    on = LaneAnswers("SqairStream", True, 0.5, False, False, 0.5, False, 0.5, None, True, 0.3, None, 10, 4.0, INF, True, "row",
                     tracklog=8, tracklog_tracks=4)
    assert (on.tracklog, on.log_L, on.log_C) == (True, 8, 4)
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError, match=r"^SqairStream.track_log: lag must be an integer in \[1, tracklog = 8\]"):
            on.track_log(lag=bad)
    for name in ("q", "r", "v0"):
        for bad in (0.0, -1.0, INF, float("nan")):
            with pytest.raises(ValueError, match=r"^SqairStream.track_log: {} must be finite and > 0".format(name)):
                on.track_log(**{name: bad})
