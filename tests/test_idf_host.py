"""No GPU: the C-ABI of IDF1 scoring (include/sqair_hip.h: sqair_set_idf, sqair_lane_idf_test, sqair_lane_idf_solve) -- exported and
declared, the binding mirrors the header's struct, the header's paragraph carries the semantics, every refusal is made before any HIP
call (dummy device pointers are enough), the IDF goes off with the score -- and the argument errors of SqairStream(score_idf=...)."""
import ctypes as C
import functools
import os

import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, c_layout, constant, dummy, err as _err, estimate, fields as header_fields, fwd_args, handle,
                            paragraph, phrases, prototype, score as _score, set_state as _state, stated_once)

NEEDED = ("box", "presence", "obj_id", "map_count")
IDF_POINTERS = _capi.IDF_TABLE + ("totals",)
_est = functools.partial(estimate, fields=NEEDED)


def _idf(P=8, without=()):
    return dummy(_capi.SqairLaneIdf, 0x9000, IDF_POINTERS, without, P=P)


def _ready(lib, h, B=4, T=2, **score):
    _state(lib, h, B)
    assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
    assert lib.sqair_set_score(h, C.byref(_score(**score)), T, B) == 0


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    names = ("sqair_set_idf", "sqair_lane_idf_test", "sqair_lane_idf_solve")
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert all(hasattr(lib, n) for n in names) and lib.sqair_abi_version() == 2
    assert all(n in _capi.EXPORTED_SYMBOLS for n in names)
    assert prototype("sqair_set_idf") == "int sqair_set_idf(SqairHandle* h, const SqairLaneIdf* idf, int T, int B)"
    assert prototype("sqair_lane_idf_test") == ("int sqair_lane_idf_test(SqairHandle* h, const float* box, const float* presence, "
                                                "const float* ids, const int32_t* map_count, int T, int B, const SqairLaneScore* score, "
                                                "const SqairLaneIdf* idf, void* stream)")
    assert prototype("sqair_lane_idf_solve") == ("int sqair_lane_idf_solve(SqairHandle* h, const SqairLaneIdf* idf, int G, int B, "
                                                 "const int32_t* close, int64_t* open, int32_t* assign, void* stream)")
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    assert constant("SQAIR_IDF_MAX_IDS") == _capi.IDF_MAX_IDS == 64
    assert constant("SQAIR_IDF_TOTALS") == len(_capi.IDF_TOTALS) == 12
    # the binding's struct mirrors the header's, field for field and in order
    fields = header_fields("SqairLaneIdf")
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairLaneIdf._fields_] == ["P"] + list(IDF_POINTERS)
    assert [ty for ty, _ in fields] == ["int32_t"] + ["int32_t*"] * len(_capi.IDF_TABLE) + ["int64_t*"]
    assert C.sizeof(_capi.SqairLaneIdf) == 8 + 8 * 10
    assert _capi.idf_shapes(3, 4, 5) == dict(col_id=(3, 5), overlap=(3, 4, 5), row_frames=(3, 4), col_frames=(3, 5), extra_frames=(3,),
                                            matched=(3, 4), frag=(3, 4), trk_state=(3, 4), frames=(3,), totals=(3, 12))
    # the totals' order is the header's
    assert ("in the order of totals: clips (1 for a clip with frames > 0), frames, trajectories, idtp, idfn, idfp, mt, pt, ml, frag"
            in paragraph())
    assert _capi.IDF_TOTALS == ("clips", "frames", "trajectories", "idtp", "idfn", "idfp", "mt", "pt", "ml", "frag", "ids", "overflow_ids")


def test_the_struct_has_the_compilers_size(tmp_path):
    """sizeof in C is what ctypes lays out."""
    got = c_layout(tmp_path, dict(SqairLaneIdf=(), SqairLaneScore=()))
    assert [got["SqairLaneIdf"][0], got["SqairLaneScore"][0]] == [C.sizeof(_capi.SqairLaneIdf), C.sizeof(_capi.SqairLaneScore)]


def test_the_header_states_the_semantics_once():
    doc = paragraph("IDF1 scoring: does an identity stay on an object", "typedef struct SqairLaneIdf")
    phrases(doc, ("k_lane_idf", "one workgroup per lane", "after k_lane_score and BEFORE the SMC resampler", "exactly one kernel node more",
                  "unchanged bit for bit", "Training passes, and a capture's eager pre-pass without effects, never run it",
                  "k_lane_idf_solve", "one wavefront per lane", "integer arithmetic", "A CLIP of lane b", "Truth identity IS the slot g",
                  "the obj_id word, or lane_id when sqair_set_score_ids(h, 1) is in force", "truth_match, which must be bound",
                  "no atomics", "P in 1..64", "-1 = free", "never read", "bit 0 = tracked at g's last present frame", "map_count != -1",
                  "takes the first free column", "UNKEYED", "the later j counts as unkeyed", "totals.overflow_ids", "EVERY pair",
                  "sq_box_iou", "not only the score's matches", "frag[g] += 1", "maximum over one-to-one assignments", "dummy-node formulation",
                  "IDFN = sum_g row_frames - IDTP", "IDFP = sum_p col_frames (used columns) + extra_frames - IDTP", "5 m >= 4 n", "5 m < n",
                  "optimal assignments tie", "sq_assign_optimal_i32", "weights below 2^30", "frees the table", "is refused (return -1",
                  "no score set", "binds no truth_match", "P outside 1..64", "another G", "Out of scope", "HOTA",
                  "more than 64 predicted ids per clip"))
    stated_once("IDF1 scoring: does an identity stay on an object")
    for name in ("DESIGN.md", "README.md"):      # they point to the header, they do not restate it
        assert "sqair_set_idf" in open(os.path.join(ROOT, name)).read(), name
    # the two places that recorded the gap point here now
    assert "are sqair_set_idf's, below" in paragraph("stream scoring: CLEAR-MOT events", "typedef struct SqairLaneScore")
    lane_h = open(os.path.join(ROOT, "sqair_amd", "csrc", "sqair_lane.h")).read()
    assert "sq_assign_optimal_i32" in lane_h and "sq_assign_keep_greedy" in lane_h


@pytest.mark.parametrize("path", LIBS)
def test_set_idf_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        B, T = 4, 2
        on = lambda idf=None, t=T, b=B: lib.sqair_set_idf(h, C.byref(idf or _idf()), t, b)
        assert lib.sqair_set_idf(None, C.byref(_idf()), T, B) == -1
        assert on() == -1 and "needs a score" in _err(lib, h)                          # no state, no estimate, no score
        _state(lib, h, B)
        assert on() == -1 and "needs a score" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
        assert on() == -1 and "needs a score" in _err(lib, h)                          # an estimate, no score
        assert lib.sqair_set_score(h, C.byref(_score(outputs=("tp", "match_iou"))), T, B) == 0
        assert on() == -1 and "truth_match" in _err(lib, h)                            # a score without truth_match
        assert lib.sqair_set_score(h, C.byref(_score()), T, B) == 0
        for t in (1, 3, 0):      # another T
            assert on(t=t) == -1 and "T = {}".format(t) in _err(lib, h) and "T = 2" in _err(lib, h)
        assert on(b=B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        for bad in (0, -1, 65, 1 << 20):
            assert on(_idf(P=bad)) == -1 and "must lie in 1..64" in _err(lib, h), bad
        for missing in IDF_POINTERS:
            assert on(_idf(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h) and missing in _err(lib, h), missing
        for P in (1, 32, 64):
            assert on(_idf(P=P)) == 0
        assert lib.sqair_set_idf(h, None, 0, 0) == 0       # NULL: off


def test_the_score_going_off_takes_the_idf_with_it():
    """The IDF can only be set while a score with truth_match is.  What switches it off cannot be seen from outside but for the node
    it launches (tests/test_idf_stream.py counts those); here: after everything that switches the score off, setting the IDF again is
    refused until the score is back, and a score re-registered without truth_match refuses it too."""
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        on = lambda T=2, b=B: lib.sqair_set_idf(h, C.byref(_idf()), T, b)
        _ready(lib, h, B)
        assert on() == 0
        assert lib.sqair_set_score(h, None, 0, 0) == 0                          # the score off
        assert on() == -1 and "needs a score" in _err(lib, h)
        assert lib.sqair_set_score(h, C.byref(_score()), 2, B) == 0 and on() == 0
        assert lib.sqair_set_score(h, C.byref(_score(outputs=("tp",))), 2, B) == 0   # re-registered without truth_match
        assert on() == -1 and "truth_match" in _err(lib, h)
        assert lib.sqair_set_score(h, C.byref(_score()), 2, B) == 0 and on() == 0
        assert lib.sqair_set_score(h, C.byref(_score(G=5)), 2, B) == 0 and on() == 0  # another G: off, and on again for the new one
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0                       # the estimate off: the score and the IDF with it
        assert on() == -1 and "needs a score" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0
        assert on() == -1 and "needs a score" in _err(lib, h)
        assert lib.sqair_set_score(h, C.byref(_score()), 2, B) == 0 and on() == 0
        assert lib.sqair_set_estimate(h, C.byref(_est()), 3, B) == 0            # another T of the estimate
        assert on(3) == -1 and "needs a score" in _err(lib, h)
        assert lib.sqair_set_score(h, C.byref(_score()), 3, B) == 0 and on(2) == -1 and on(3) == 0
        assert lib.sqair_set_estimate(h, C.byref(_est(without=("map_count",))), 3, B) == 0   # an estimate the score cannot read
        assert on(3) == -1 and "needs a score" in _err(lib, h)
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0              # the state off
        assert on(3) == -1 and "needs a score" in _err(lib, h)
        _ready(lib, h, B)
        assert on() == 0
        _state(lib, h, B + 1)                                                   # another B
        assert on(2, B + 1) == -1 and "needs a score" in _err(lib, h)


def test_training_calls_never_run_the_idf():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _ready(lib, h, B)
        assert lib.sqair_set_idf(h, C.byref(_idf()), 2, B) == 0
        assert lib.sqair_forward_train(*fwd_args(h, B, T=2)) == -1
        assert "carried state" in _err(lib, h)


@pytest.mark.parametrize("path", LIBS)
def test_kernel_entry_point_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        good = dict(box=DUMMY, presence=DUMMY, ids=DUMMY, map_count=DUMMY, T=1, B=3)
        order = ("box", "presence", "ids", "map_count", "T", "B")
        ref = lambda x: C.byref(x) if x is not None else None
        call = lambda sc, idf, **kw: lib.sqair_lane_idf_test(h, *[dict(good, **kw)[k] for k in order], ref(sc), ref(idf), DUMMY)
        assert lib.sqair_lane_idf_test(None, *[good[k] for k in order], C.byref(_score()), C.byref(_idf()), DUMMY) == -1
        for kw in (dict(box=None), dict(presence=None), dict(ids=None), dict(map_count=None), dict(T=0), dict(T=65536), dict(B=0)):
            assert call(_score(), _idf(), **kw) == -1 and "sqair_lane_idf_test" in _err(lib, h), kw
        assert call(None, _idf()) == -1 and call(_score(), None) == -1
        for bad in (0.0, 1.5, float("nan")):
            assert call(_score(iou_min=bad), _idf()) == -1 and "iou_min" in _err(lib, h)
        for bad in (0, 17):
            assert call(_score(G=bad), _idf()) == -1 and "1..16" in _err(lib, h)
        for missing in ("truth_box", "truth_present", "truth_valid"):
            assert call(_score(without=(missing,)), _idf()) == -1 and "must not be NULL" in _err(lib, h)
        assert call(_score(outputs=("tp",)), _idf()) == -1 and "truth_match" in _err(lib, h)
        for bad in (0, 65):
            assert call(_score(), _idf(P=bad)) == -1 and "1..64" in _err(lib, h)
        for missing in IDF_POINTERS:
            assert call(_score(), _idf(without=(missing,))) == -1 and missing in _err(lib, h)
        # the solve
        solve = lambda idf, G=4, B=3: lib.sqair_lane_idf_solve(h, ref(idf), G, B, None, None, None, DUMMY)
        assert lib.sqair_lane_idf_solve(None, C.byref(_idf()), 4, 3, None, None, None, DUMMY) == -1
        assert solve(None) == -1 and "sqair_lane_idf_solve" in _err(lib, h)
        for bad in (0, 17):
            assert solve(_idf(), G=bad) == -1 and "1..16" in _err(lib, h)
        assert solve(_idf(), B=0) == -1 and "B = 0" in _err(lib, h)
        for bad in (0, 65):
            assert solve(_idf(P=bad)) == -1 and "1..64" in _err(lib, h)
        for missing in IDF_POINTERS:
            assert solve(_idf(without=(missing,))) == -1 and missing in _err(lib, h)


def test_stream_argument_errors():
    """The IDF's arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    with pytest.raises(ValueError, match=r"^SqairStream: score_idf is for a stream with score=True"):
        SqairStream(Core(), 2, estimate=True, score_idf=True)
    with pytest.raises(ValueError, match=r"^SqairStream: score is for a stream with estimate=True"):
        SqairStream(Core(), 2, score=True, score_idf=True)
    for bad in (0, 65, -3, 2.5, True, "4", None):
        with pytest.raises(ValueError, match=r"^SqairStream: score_idf_ids must be an integer in \[1, 64\]"):
            SqairStream(Core(), 2, estimate=True, score=True, score_idf=True, score_idf_ids=bad)
