"""No GPU: the C-ABI of track log stitching (include/sqair_hip.h: sqair_lane_tracklog_stitch) -- exported and declared in all three
libraries, the binding mirrors the header's struct, the track log stitching paragraph carries the semantics, every refusal of the entry
is made before any HIP call (dummy device pointers are enough) -- and the argument errors of ``track_log(stitch=True)``."""
import ctypes as C
import inspect
import os

import pytest

from sqair_amd import _capi
from sqair_amd.lane import LaneAnswers
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, c_layout, dummy, err as _err, fields as header_fields, handle, paragraph, phrases, prototype,
                            stated_once, constant)

INF = float("inf")
NAN = float("nan")
N = 3
NAME = "sqair_lane_tracklog_stitch"
FIELDS = ["gate", "max_gap", "link_next", "link_d2", "link_gap", "root", "n_links"]


def _log(L=8, without=()):
    return dummy(_capi.SqairLaneTrackLog, 0xa000, _capi.TRACKLOG_FIELDS, without, L=L)


def _table(base=0xb000, without=()):
    return dummy(_capi.SqairTrackLogOut, base, _capi.TRACKLOG_OUT_FIELDS, without)


def _stitch(gate=3.5, max_gap=8, without=()):
    return dummy(_capi.SqairTrackLogStitch, 0xe000, _capi.TRACKLOG_STITCH_FIELDS, without, gate=gate, max_gap=max_gap)


def test_the_symbol_is_exported_and_declared_and_the_abi_is_unchanged(tmp_path):
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, NAME) and lib.sqair_abi_version() == 2
    assert NAME in _capi.EXPORTED_SYMBOLS and _capi.ABI_VERSION == 2
    assert prototype(NAME) == (
        "int sqair_lane_tracklog_stitch(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table, const void* work, "
        "int lag, int C, int N, int B, float q, float r, float v0_var, const SqairTrackLogStitch* stitch, "
        "const SqairTrackLogOut* stitched, void* work_out, void* stream)")
    assert header_fields("SqairTrackLogStitch") == [
        ("float", "gate"), ("int32_t", "max_gap"), ("int32_t*", "link_next"), ("float*", "link_d2"), ("int32_t*", "link_gap"),
        ("int32_t*", "root"), ("int32_t*", "n_links")]
    assert [n for n, _ in _capi.SqairTrackLogStitch._fields_] == FIELDS
    lay = c_layout(tmp_path, {"SqairTrackLogStitch": FIELDS})
    offsets = [getattr(_capi.SqairTrackLogStitch, n).offset for n in FIELDS]
    assert lay["SqairTrackLogStitch"] == (C.sizeof(_capi.SqairTrackLogStitch), offsets) == (48, [0, 4, 8, 16, 24, 32, 40])
    assert _capi.TRACKLOG_STITCH_FIELDS == tuple(FIELDS[2:])
    assert _capi.TRACKLOG_STITCH_LINKS == dict(next="link_next", d2="link_d2", gap="link_gap", root="root", n_links="n_links")
    assert [_capi.field_dtype("SqairTrackLogStitch", n) for n in FIELDS[2:]] == ["int32", "float32", "int32", "int32", "int32"]
    assert _capi.tracklog_stitch_shapes(2, 5) == dict(link_next=(2, 5), link_d2=(2, 5), link_gap=(2, 5), root=(2, 5), n_links=(2,))


def test_the_header_states_the_semantics_once():
    doc = paragraph("track log stitching: join a track's fragments with hindsight", "typedef struct SqairTrackLogStitch")
    phrases(doc, ("the track log stitching paragraph", "stand-alone, capturable call", "one launch of k_lane_tracklog_stitch",
                  "one workgroup of 256 threads per lane", "it registers nothing", "no pass runs it", "it reads nothing of a previous call",
                  "it writes only its outputs", "The handle gives the error text only",
                  "`table` and `work` exactly as sqair_lane_tracklog_smooth left them for the same lag, C, N and B",
                  "No pass may have run between the solve and the stitch", "stitch->gate, finite and > 0", "stitch->max_gap in 0..lag",
                  "1. Fragments.", "The kept columns c with track_id[b,c] >= 0", "the first and the last frame with state[f,b,c] != 0",
                  "2. Candidates.", "f1_a < f0_b", "len0[b,cb] == 1", "gap <= max_gap", "that COUNT in the solve's sense",
                  "3. Distance", "filt[f1_a,b,a,axis,:] coasted with P", "sq_kf_predict, called, not restated",
                  "once per frame that counts in (f1_a, f0_b]", "frames that do not count do not step",
                  "smooth[f0_b,b,cb,axis,:]", "backward-informed birth state", "The two rest on disjoint measurements",
                  "A = Aa + Ab; Bm = Ba + Bb; Cm = Ca + Cb; det = fmaf(A, Cm, -(Bm Bm)); dp = pb - pa; dv = vb - va",
                  "num = fmaf(A dv, dv, fmaf(-2, Bm dv, Cm dp) dp); d2_axis = num / det", "d2 = d2_y + d2_x, four degrees of freedom",
                  "ELIGIBLE when det_y > 0, det_x > 0 and d2 <= gate gate", "A NaN never passes",
                  "4. Assignment over the C x C table in LDS (at most 16 KiB)", "rows = predecessors, columns = successors",
                  "weight 2^28 + q for an eligible pair", "__float2int_rn((1 - d2 / (gate gate)) * 1048576.0f)", "-1 for every other pair",
                  "Wave 0 calls sq_assign_optimal_i32", "64 pairs x 2^20 < 2^28", "cardinality first", "below 2^30, the solver's exact range",
                  "deterministic, not restated as a rule", "5. Chains.", "at most one successor and one predecessor",
                  "A chain's root is its first fragment", "6. The stitched table", "one column per chain", "track_id = the root's id, ascending",
                  "len0 the root's", "n_tracks = the solve's minus the number of links", "frame_index copied",
                  "work_out[f,c'] = the `work` word of the chain's fragment whose span f0..f1 holds f", "-1 elsewhere",
                  "ONE device function, sq_tracklog_walk, called by both kernels", "a bridged frame that counts is state 2",
                  "one that does not count is state 3", "what the solve would have written had the identity kept one id",
                  "7. Link outputs, every word written", "link_next [B,C] int32", "link_d2 [B,C] fp32", "link_gap [B,C] int32",
                  "root [B,C] int32", "n_links [B] int32",
                  "Refused (return -1, text in sqair_last_error, before any HIP call)", "a NULL log, table, work, stitch, stitched or work_out",
                  "what sqair_set_tracklog refuses for log", "lag outside 1..L", "C outside 1..64", "N outside 1..16", "B < 1",
                  "any of q, r, v0_var not finite and positive", "gate not finite and positive", "max_gap outside 0..lag",
                  "sharing its pointer with a field of the table or with work",
                  "Out of scope", "re-linking inside a fragment", "splitting a track", "appearance in the distance",
                  "fitting on the stitched table", "links to tracks not among the C kept columns", "a stated tie rule",
                  "stitching inside the pass or feeding links back to the identity kernel", "filtering h, w", "training passes"))
    stated_once("track log stitching: join a track's fragments with hindsight")
    assert constant("SQAIR_ABI_VERSION") == 2
    for name in ("DESIGN.md", "README.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "sqair_lane_tracklog_stitch" in text and "k_lane_tracklog_stitch" in text and "stitch=True" in text, name
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert readme.index("**Motion calibration**") < readme.index("**Track log stitching**") < readme.index("**IDF1 scoring**")
    assert "## 3v. Track log stitching" in open(os.path.join(ROOT, "DESIGN.md")).read()


@pytest.mark.parametrize("path", LIBS)
def test_the_entrys_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        good = dict(log=_log(L=8), table=_table(), work=DUMMY, lag=8, C=4, N=N, B=2, q=0.25, r=1.0, v0=16.0, stitch=_stitch(),
                    stitched=_table(0xc000), work_out=C.c_void_p(0x2000))

        def call(hh=h, **kw):
            a = dict(good, **kw)
            ref = lambda v: C.byref(v) if v is not None else None
            return lib.sqair_lane_tracklog_stitch(hh, ref(a["log"]), ref(a["table"]), a["work"], a["lag"], a["C"], a["N"], a["B"], a["q"],
                                                  a["r"], a["v0"], ref(a["stitch"]), ref(a["stitched"]), a["work_out"], DUMMY)
        assert call(hh=None) == -1
        for kw in (dict(log=None), dict(table=None), dict(work=None), dict(stitch=None), dict(stitched=None), dict(work_out=None)):
            assert call(**kw) == -1 and NAME + ": log, table, work, stitch, stitched and work_out must not be NULL" in _err(lib, h), kw
        for L in (0, 4097):                                                             # what sqair_set_tracklog refuses for the log
            assert call(log=_log(L=L)) == -1 and "L = {} must lie in 1..4096".format(L) in _err(lib, h)
        for missing in _capi.TRACKLOG_FIELDS:
            assert call(log=_log(without=(missing,))) == -1 and "count, log_valid, log_id, log_len and log_box must not be NULL" in _err(lib, h)
        for lag in (0, -1, 9, 4097):
            assert call(lag=lag) == -1 and NAME + ": lag" in _err(lib, h) and "must lie in 1..L" in _err(lib, h), lag
        for Cn in (0, -1, 65):
            assert call(C=Cn) == -1 and "C must lie in 1..64" in _err(lib, h)
        for n in (0, -1, 17):
            assert call(N=n) == -1 and "N must lie in 1..16" in _err(lib, h)
        for b in (0, -3):
            assert call(B=b) == -1 and "B = {} must be >= 1".format(b) in _err(lib, h)
        for bad in (0.0, -1.0, INF, NAN):
            for name in ("q", "r", "v0"):
                assert call(**{name: bad}) == -1 and NAME + ": {} must be finite and > 0".format(dict(v0="v0_var").get(name, name)) in _err(lib, h)
            assert call(stitch=_stitch(gate=bad)) == -1 and NAME + ": gate must be finite and > 0" in _err(lib, h), bad
        for bad in (-1, 9, 1 << 20):
            assert call(stitch=_stitch(max_gap=bad)) == -1 and "max_gap = {} must lie in 0..lag = 8".format(bad) in _err(lib, h)
        for missing in _capi.TRACKLOG_STITCH_TABLE:
            assert call(table=_table(without=(missing,))) == -1 and "the table's track_id, n_tracks, len0, frame_index, state, filt and " \
                "smooth must not be NULL" in _err(lib, h), missing
        for missing in _capi.TRACKLOG_OUT_FIELDS:
            assert call(stitched=_table(0xc000, without=(missing,))) == -1 and "stitched's track_id, n_tracks, len0, frame_index, state, " \
                "size, filt and smooth must not be NULL" in _err(lib, h), missing
        for missing in _capi.TRACKLOG_STITCH_FIELDS:
            assert call(stitch=_stitch(without=(missing,))) == -1 and "link_next, link_d2, link_gap, root and n_links must not be NULL" \
                in _err(lib, h), missing
        shared = "stitched and work_out must not share a pointer with table or work"
        assert call(stitched=_table()) == -1 and shared in _err(lib, h)                 # the table itself
        assert call(work_out=DUMMY) == -1 and shared in _err(lib, h)                    # work itself
        one = _table(0xc000)
        one.smooth = good["table"].smooth
        assert call(stitched=one) == -1 and shared in _err(lib, h)                      # one field of the table
        assert call(work_out=C.c_void_p(good["table"].state)) == -1 and shared in _err(lib, h)


def _answers(tracklog=8, **kw):
    base = ("SqairStream", True, 0.5, False, False, 0.5)
    rest = (True, 0.3, None, 10, 4.0, INF, True, "row")
    return LaneAnswers(*base, False, 0.5, None, *rest, motion=False, tracklog=tracklog, tracklog_tracks=4, **kw)


def test_track_log_stitch_argument_errors():
    """The arguments are checked before the core is touched (these objects have none)."""
    for cls in (SqairStream, LaneAnswers):
        p = inspect.signature(cls.track_log).parameters
        assert (p["stitch"].default, p["stitch_gate"].default, p["stitch_max_gap"].default) == (False, 3.5, None), cls
    with pytest.raises(ValueError, match=r"^SqairStream.track_log: the stream keeps no track log"):
        _answers(tracklog=None).track_log(stitch=True)
    la = _answers()
    for bad in (0.0, -1.0, INF, NAN, "x", None):
        with pytest.raises(ValueError, match=r"^SqairStream.track_log: stitch_gate must be finite and > 0"):
            la.track_log(stitch=True, stitch_gate=bad)
    for bad in (-1, 9, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"^SqairStream.track_log: stitch_max_gap must be an integer in \[0, lag = 8\]"):
            la.track_log(stitch=True, stitch_max_gap=bad)
    with pytest.raises(ValueError, match=r"^SqairStream.track_log: stitch_max_gap must be an integer in \[0, lag = 5\]"):
        la.track_log(lag=5, stitch=True, stitch_max_gap=6)
    with pytest.raises(ValueError, match=r"^SqairStream.track_log: score=True is for a stream that keeps the log's truth"):
        la.track_log(stitch=True, score=True)
