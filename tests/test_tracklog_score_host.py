"""No GPU: the C-ABI of track log scoring (include/sqair_hip.h: sqair_lane_tracklog_score) -- exported and declared, the binding
mirrors the header's structs and constants, the track log scoring paragraph carries the semantics and the older "out of scope"
sentences point to it, every refusal of the entry is made before any HIP call (dummy device pointers are enough) -- and the argument
errors of SqairStream(tracklog_truth=...), ``step(truth=...)`` and ``track_log(score=True)``."""
import ctypes as C
import os

import pytest

from sqair_amd import _capi
from sqair_amd.lane import LaneAnswers
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, c_layout, constant, dummy, err as _err, fields as header_fields, handle, paragraph, phrases,
                            prototype, stated_once)

INF = float("inf")
N = 3
TABLE = ("track_id", "frame_index", "state", "size", "filt", "smooth")
VIEWS = ("filtered", "smooth", "filtered_filled", "smooth_filled")
COUNTS = ("frames", "frames_invalid", "truth", "tp", "fn", "fp", "idsw", "gap_tp", "gap_fp", "nees_n", "gap_nees_n", "idtp", "idfn", "idfp")
SUMS = ("iou_sum", "err_sum", "nees_sum", "gap_err_sum", "gap_nees_sum")


def _log(L=8, without=()):
    return dummy(_capi.SqairLaneTrackLog, 0xa000, _capi.TRACKLOG_FIELDS, without, L=L)


def _table(without=()):
    return dummy(_capi.SqairTrackLogOut, 0xb000, _capi.TRACKLOG_OUT_FIELDS, without)


def _truth(G=4, without=()):
    return dummy(_capi.SqairTrackLogTruth, 0xc000, _capi.TRACKLOG_TRUTH_FIELDS, without, G=G)


def _score(iou_min=0.5, without=()):
    return dummy(_capi.SqairTrackLogScore, 0xd000, _capi.TRACKLOG_SCORE_REQUIRED + _capi.TRACKLOG_SCORE_FIELDS, without, iou_min=iou_min)


def test_the_symbol_is_exported_and_declared_and_the_abi_is_unchanged(tmp_path):
    name = "sqair_lane_tracklog_score"
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, name) and lib.sqair_abi_version() == 2
    assert name in _capi.EXPORTED_SYMBOLS and _capi.ABI_VERSION == 2
    assert prototype(name) == (
        "int sqair_lane_tracklog_score(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table, "
        "const SqairTrackLogTruth* truth, const SqairTrackLogScore* score, int lag, int C, int B, int match, void* stream)")
    truth = header_fields("SqairTrackLogTruth")
    assert truth == [("int32_t", "G"), ("const float*", "truth_box"), ("const int32_t*", "truth_present"), ("const int32_t*", "truth_valid")]
    assert [n for n, _ in _capi.SqairTrackLogTruth._fields_] == ["G"] + list(_capi.TRACKLOG_TRUTH_FIELDS)
    score = header_fields("SqairTrackLogScore")
    assert score == [("float", "iou_min"), ("int64_t*", "counts"), ("double*", "sums"), ("int32_t*", "assign"), ("int32_t*", "match"),
                     ("float*", "match_iou")]
    assert [n for n, _ in _capi.SqairTrackLogScore._fields_] == ["iou_min"] + list(_capi.TRACKLOG_SCORE_REQUIRED + _capi.TRACKLOG_SCORE_FIELDS)
    lay = c_layout(tmp_path, {"SqairTrackLogTruth": ["G", "truth_box", "truth_valid"], "SqairTrackLogScore": ["iou_min", "counts", "match_iou"]})
    assert lay["SqairTrackLogTruth"] == (C.sizeof(_capi.SqairTrackLogTruth), [0, 8, 24]) == (32, [0, 8, 24])
    assert lay["SqairTrackLogScore"] == (C.sizeof(_capi.SqairTrackLogScore), [0, 8, 40]) == (48, [0, 8, 40])
    assert constant("SQAIR_TRACKLOG_SCORE_VIEWS") == 4 and _capi.TRACKLOG_SCORE_VIEWS == VIEWS
    assert constant("SQAIR_TRACKLOG_SCORE_COUNTS") == 14 and _capi.TRACKLOG_SCORE_COUNTS == COUNTS
    assert constant("SQAIR_TRACKLOG_SCORE_SUMS") == 5 and _capi.TRACKLOG_SCORE_SUMS == SUMS
    assert _capi.TRACKLOG_SCORE_TABLE == TABLE and set(TABLE) <= set(_capi.TRACKLOG_OUT_FIELDS)
    assert _capi.TRACKLOG_SCORE_INT_FIELDS == ("assign", "match")
    assert _capi.field_dtype("SqairTrackLogScore", "counts") == "int64" and _capi.field_dtype("SqairTrackLogScore", "sums") == "float64"
    assert _capi.tracklog_truth_shapes(5, 2, 3) == dict(truth_box=(5, 2, 3, 4), truth_present=(5, 2, 3), truth_valid=(5, 2))
    assert _capi.tracklog_score_shapes(5, 2, 3) == dict(counts=(2, 4, 14), sums=(2, 4, 5), assign=(4, 2, 3), match=(4, 5, 2, 3),
                                                        match_iou=(4, 5, 2, 3))


def test_the_header_states_the_semantics_once():
    doc = paragraph("track log scoring: the solve's trajectories against ground-truth boxes", "#define SQAIR_TRACKLOG_SCORE_VIEWS")
    phrases(doc, ("the track log scoring paragraph", "stand-alone, capturable call", "one launch of k_lane_tracklog_score",
                  "one workgroup of four wavefronts per lane", "it registers nothing", "no pass runs it", "it writes only `score`",
                  "pure function of its inputs", "no in/out accumulators", "the windows of successive calls overlap",
                  "summing over calls is the caller's business", "The handle gives the error text only",
                  "`table` (read-only) is what sqair_lane_tracklog_smooth wrote for the same lag, C and B",
                  "track_id, frame_index, state, size, filt and smooth are read", "`log` gives L, count and log_valid",
                  "a non-finite frame is told from an empty one", "WINDOW ORDER, oldest to newest", "as for sqair_lane_traj_score",
                  "the caller brings the truth of the table's frames", "G in 1..16", "truth_box [lag,B,G,4] fp32 (y, x, h, w)",
                  "truth_present [lag,B,G] and truth_valid [lag,B] int32", "truth identity IS the slot g", "score->iou_min in (0, 1]",
                  "1. Views", "src = v & 1 (0: filt, 1: smooth), fill = v >> 1", "state[f,b,c] == 1",
                  "fill is set and state[f,b,c] == 2", "(fmaf(-0.5f, h, p_y), fmaf(-0.5f, w, p_x), h, w)",
                  "p the word 0 of src[f,b,c,axis,:]", "(h, w) = size[f,b,c,:]", "View 0 is what a causal tracker reported",
                  "view 3 is what the MOTChallenge rows of the log export", "Wavefront v owns view v",
                  "2. Frames", "frame_index[f,b] >= 0", "its record (frame_index mod L) has log_valid != 0", "truth_valid[f,b] != 0",
                  "counts one frames_invalid and nothing else", "every other frame changes nothing", "-1 (match) and 0 (match_iou)",
                  "3. Per scored frame and view, frames in ascending order", "holes are allowed on both sides",
                  "sq_box_iou", "on the fp32 words", "sq_assign_keep_greedy (match == 0)", "sq_assign_keep_optimal (match == 1",
                  "N := C, col_id[c] = track_id[b,c] and keep_id[g] = last[v][g]", "-1 at the start of EVERY call",
                  "exactly as point 4 of the stream scoring paragraph defines them", "tp = matched pairs",
                  "fn = present truths unmatched", "fp = present columns unclaimed",
                  "idsw += [last[v][g] >= 0 and last[v][g] != id], then last[v][g] = id", "match[v,f,b,g] = c",
                  "match_iou[v,f,b,g] = the pair's IoU",
                  "4. For each matched pair (g, c), in fp32 and in this order", "ty = fmaf(0.5f, th, t_y); tx = fmaf(0.5f, tw, t_x)",
                  "dy = ty - p_y; dx = tx - p_x; err = sqrtf(fmaf(dy, dy, dx * dx))", "both Ppp_y > 0 and Ppp_x > 0",
                  "a NaN or a non-positive variance is not counted", "nees = dy * dy / Ppp_y + dx * dx / Ppp_x", "counts in nees_n",
                  "its expectation is 2 for an honest sigma", "gap_tp, gap_err_sum", "gap_nees_sum and gap_nees_n",
                  "a present, unclaimed column at state 2 counts in gap_fp",
                  "5. IDF over the window, per view", "ov[g][c] (int32)", "no one-to-one", "the overlap table of Ristani et al.",
                  "sq_assign_optimal_i32(ov, C, G, C, .)", "idtp = the optimum", "idfn = (present truths over the scored frames) - idtp",
                  "idfp = (present columns over the scored frames) - idtp", "assign[v,b,g] = the column assigned to g",
                  "optimal assignments tie, the figures do not", "<= lag <= 4096", "the solver's exact range",
                  "6. Outputs", "counts [B,4,14] int64",
                  "frames (scored), frames_invalid, truth, tp, fn, fp, idsw, gap_tp, gap_fp, nees_n, gap_nees_n, idtp, idfn, idfp",
                  "sums [B,4,5] fp64 = iou_sum, err_sum, nees_sum, gap_err_sum, gap_nees_sum",
                  "converted to fp64 and added by one thread, g in index order, frames in order", "no float atomics",
                  "a replayed graph gives the bits of an eager call", "every word of them is written",
                  "assign [4,B,G], match and match_iou [4,lag,B,G] are optional",
                  "7. Refused (return -1, text in sqair_last_error, before any HIP call)", "a NULL log, table, truth or score",
                  "what sqair_set_tracklog refuses for log", "a NULL track_id, frame_index, state, size, filt or smooth of the table",
                  "a NULL truth_box, truth_present or truth_valid", "a NULL counts or sums", "lag outside 1..L", "C outside 1..64",
                  "G outside 1..16", "B < 1", "iou_min NaN or outside (0, 1]", "match other than 0 or 1",
                  "Out of scope", "sums that persist over windows", "HOTA of the log", "scoring per particle row", "filtering h, w",
                  "truth identities other than the slot"))
    stated_once("track log scoring: the solve's trajectories against ground-truth boxes")
    # the three older sentences stay and point here
    log = paragraph("the track log: trajectories per lane_id", "#define SQAIR_TRACKLOG_MAX_FRAMES")
    phrases(log, ("Out of scope", "scoring the log against truth here (that is sqair_lane_tracklog_score's, next)"))
    for name in ("DESIGN.md", "README.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "scoring the log against truth" in text and "sqair_lane_tracklog_score" in text, name
        assert "k_lane_tracklog_score" in text and "tracklog_truth" in text, name


@pytest.mark.parametrize("path", LIBS)
def test_the_entrys_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        good = dict(log=_log(L=8), table=_table(), truth=_truth(), score=_score(), lag=8, C=4, B=2, match=0)

        def call(**kw):
            a = dict(good, **kw)
            ref = lambda v: C.byref(v) if v is not None else None
            return lib.sqair_lane_tracklog_score(h, ref(a["log"]), ref(a["table"]), ref(a["truth"]), ref(a["score"]), a["lag"], a["C"],
                                                 a["B"], a["match"], DUMMY)
        assert lib.sqair_lane_tracklog_score(None, C.byref(good["log"]), C.byref(good["table"]), C.byref(good["truth"]),
                                             C.byref(good["score"]), 8, 4, 2, 0, DUMMY) == -1
        for kw in (dict(log=None), dict(table=None), dict(truth=None), dict(score=None)):
            assert call(**kw) == -1 and "sqair_lane_tracklog_score: log, table, truth and score must not be NULL" in _err(lib, h), kw
        for L in (0, 4097):                                                             # what sqair_set_tracklog refuses for the log
            assert call(log=_log(L=L)) == -1 and "L = {} must lie in 1..4096".format(L) in _err(lib, h)
        for missing in _capi.TRACKLOG_FIELDS:
            assert call(log=_log(without=(missing,))) == -1 and "count, log_valid, log_id, log_len and log_box must not be NULL" in _err(lib, h)
        for lag in (0, -1, 9, 4097):
            assert call(lag=lag) == -1 and "lag = {} must lie in 1..L = 8".format(lag) in _err(lib, h), lag
        for Cn in (0, -1, 65):
            assert call(C=Cn) == -1 and "C = {} must lie in 1..64".format(Cn) in _err(lib, h)
        for G in (0, -1, 17):
            assert call(truth=_truth(G=G)) == -1 and "G = {} must lie in 1..16".format(G) in _err(lib, h)
        for b in (0, -3):
            assert call(B=b) == -1 and "B = {} must be >= 1".format(b) in _err(lib, h)
        for bad in (0.0, -0.5, 1.5, INF, float("nan")):
            assert call(score=_score(iou_min=bad)) == -1 and "iou_min" in _err(lib, h), bad
        for m in (-1, 2, 7):
            assert call(match=m) == -1 and "match = {} must be 0 (greedy) or 1 (optimal)".format(m) in _err(lib, h)
        for missing in TABLE:
            assert call(table=_table(without=(missing,))) == -1 and "track_id, frame_index, state, size, filt and smooth must not be NULL" in _err(lib, h)
        for missing in _capi.TRACKLOG_TRUTH_FIELDS:
            assert call(truth=_truth(without=(missing,))) == -1 and "truth_box, truth_present and truth_valid must not be NULL" in _err(lib, h)
        for missing in _capi.TRACKLOG_SCORE_REQUIRED:
            assert call(score=_score(without=(missing,))) == -1 and "counts and sums must not be NULL" in _err(lib, h)


def test_stream_argument_errors():
    """The arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    ident = dict(estimate=True, identity=True)
    for kw in (dict(), dict(estimate=True), ident):
        with pytest.raises(ValueError, match=r"^SqairStream: tracklog_truth is for a stream with tracklog=L"):
            SqairStream(Core(), 2, tracklog_truth=2, **kw)
    for bad in (0, -1, 17, 2.0, True, "2"):
        with pytest.raises(ValueError, match=r"^SqairStream: tracklog_truth must be an integer in \[1, 16\]"):
            SqairStream(Core(), 2, tracklog=8, tracklog_truth=bad, **ident)
    with pytest.raises(ValueError, match=r"^SqairStream: tracklog_truth must equal score_truth"):
        SqairStream(Core(), 2, tracklog=8, tracklog_truth=3, score=True, score_truth=4, **ident)
    base = ("SqairStream", True, 0.5, False, False, 0.5)
    rest = (True, 0.3, None, 10, 4.0, INF, True, "row")

    class N3(object):
        N = 3
    on = LaneAnswers(*base, True, 0.5, None, *rest, tracklog=8, tracklog_tracks=4, tracklog_truth=2)      # score_truth defaults to the core's N
    with pytest.raises(ValueError, match=r"^SqairStream: tracklog_truth must equal score_truth"):
        on.size(N3())
    ok = LaneAnswers(*base, True, 0.5, None, *rest, tracklog=8, tracklog_tracks=4, tracklog_truth=3)
    ok.size(N3())
    assert (ok.G, ok.log_G) == (3, 3)
    # truth without a score and without the log's truth: the old refusal stays; with tracklog_truth it is taken
    neither = LaneAnswers(*base, False, 0.5, None, *rest, tracklog=8, tracklog_tracks=4)
    with pytest.raises(ValueError, match=r"^SqairStream.step: truth is for a stream with score=True"):
        neither.check_truth(dict(box=[], present=[]))
    with pytest.raises(ValueError, match=r"^SqairStream.track_log: score=True is for a stream that keeps the log's truth .*tracklog_truth=G"):
        neither.track_log(score=True)
    import torch
    kept = LaneAnswers(*base, False, 0.5, None, *rest, tracklog=8, tracklog_tracks=4, tracklog_truth=2)
    kept.T, kept.B = 1, 2
    box, present, valid = kept.check_truth(dict(box=torch.zeros(2, 2, 4), present=torch.ones(2, 2)))
    assert box.shape == (1, 2, 2, 4) and present.dtype == torch.int32 and valid.shape == (1, 2)
    with pytest.raises(ValueError, match=r"^SqairStream.step: truth\['box'\] of shape"):
        kept.check_truth(dict(box=torch.zeros(2, 3, 4), present=torch.ones(2, 3)))
    for bad in (0.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"^SqairStream.track_log: score_iou must lie in \(0, 1\]"):
            kept.track_log(score=True, score_iou=bad)
    with pytest.raises(ValueError, match=r"^SqairStream.track_log: score_match must be 'greedy' or 'optimal'"):
        kept.track_log(score=True, score_match="best")
