"""No GPU: the C-ABI of stream scoring (include/sqair_hip.h: sqair_set_score, sqair_lane_score_test) -- exported and declared, the
binding mirrors the header's struct, the header's paragraph carries the semantics, every refusal is made before any HIP call (dummy
device pointers are enough), the score goes off with the estimate and the state -- and the argument errors of SqairStream(score=...)."""
import ctypes as C
import functools
import os

import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, constant, err as _err, estimate, fields as header_fields, fwd_args as _fwd_args, handle,
                            paragraph, phrases, prototype, score as _score, set_state as _state, stated_once)

NEEDED = ("box", "presence", "obj_id", "map_count")
_est = functools.partial(estimate, fields=NEEDED)


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, "sqair_set_score") and hasattr(lib, "sqair_lane_score_test") and lib.sqair_abi_version() == 2
    assert "sqair_set_score" in _capi.EXPORTED_SYMBOLS and "sqair_lane_score_test" in _capi.EXPORTED_SYMBOLS
    assert prototype("sqair_set_score") == "int sqair_set_score(SqairHandle* h, const SqairLaneScore* score, int T, int B)"
    assert prototype("sqair_lane_score_test") == ("int sqair_lane_score_test(SqairHandle* h, const float* box, const float* presence, "
                                                  "const float* obj_id, const int32_t* map_count, int T, int B, "
                                                  "const SqairLaneScore* score, void* stream)")
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    assert constant("SQAIR_SCORE_MAX_TRUTH") == _capi.SCORE_MAX_TRUTH
    assert constant("SQAIR_SCORE_COUNTS") == len(_capi.SCORE_COUNTS)
    # the binding's struct mirrors the header's, field for field and in order
    fields = header_fields("SqairLaneScore")
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairLaneScore._fields_]
    assert [n for _, n in fields] == ["iou_min", "G"] + list(_capi.SCORE_INPUTS) + list(_capi.SCORE_FIELDS)
    assert [n for ty, n in fields if ty == "int32_t*"] == ["last_id"] + list(_capi.SCORE_INT_FIELDS)
    types = {n: ty for ty, n in fields}
    assert types["counts"] == "int64_t*" and types["iou_sum"] == "double*" and types["truth_box"] == "const float*" and types["G"] == "int32_t"
    assert C.sizeof(_capi.SqairLaneScore) == 8 + 8 * 12
    assert _capi.score_shapes(2, 3, 5) == dict(truth_match=(2, 3, 5), match_iou=(2, 3, 5), tp=(2, 3), fn=(2, 3), fp=(2, 3), idsw=(2, 3))
    # the counters' order is the header's
    assert "counts [B,9] int64: frames (scored), frames_invalid, truth, tp, fn, fp, idsw, count_hit, count_abs_err" in paragraph()
    assert _capi.SCORE_COUNTS == ("frames", "frames_invalid", "truth", "tp", "fn", "fp", "idsw", "count_hit", "count_abs_err")


def test_the_header_states_the_semantics_once():
    doc = paragraph("stream scoring: CLEAR-MOT events", "typedef struct SqairLaneScore")
    phrases(doc, ("k_lane_score", "one workgroup per lane", "after k_lane_estimate (and after k_lane_layers if on)", "BEFORE the SMC resampler",
                  "exactly one kernel node more", "unchanged bit for bit", "Training passes never run it", "does not read the records again",
                  "truth identity IS the slot g", "truth_valid [T,B] int32", "G in 1..16", "Non-finite lanes", "map_count == -1",
                  "frames_invalid", "Holes are allowed", "sq_box_iou", "the first unclaimed present j whose obj_id word equals last_id[b,g]",
                  "greedy one-to-one", "ties to the smallest g, then the smallest j", "A NaN never wins", "unmatched g keep their memory",
                  "match_iou[t,b,g]", "truth_match[t,b,g]", "count_hit += [map_count == n_truth]", "count_abs_err += |map_count - n_truth|",
                  "updated in place", "iou_sum [B] fp64", "g in index order, frames in order, from one thread", "no float atomics", "Coasted",
                  "the per-frame outputs are optional", "Refused", "a pass of another T", "Out of scope", "optimal (Hungarian) assignment",
                  "IDF1", "scoring per particle row", "scoring of forecasts or lane tracks", "training passes"))
    stated_once("stream scoring: CLEAR-MOT events")
    for name in ("DESIGN.md", "README.md"):      # they point to the header, they do not restate it
        assert "sqair_set_score" in open(os.path.join(ROOT, name)).read(), name


@pytest.mark.parametrize("path", LIBS)
def test_set_score_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        B, T = 4, 2
        on = lambda sc=None, t=T, b=B: lib.sqair_set_score(h, C.byref(sc or _score()), t, b)
        assert lib.sqair_set_score(None, C.byref(_score()), T, B) == -1
        assert on() == -1 and "sqair_set_estimate" in _err(lib, h)                    # no state, no estimate
        _state(lib, h, B)
        assert on() == -1 and "needs an estimate" in _err(lib, h)                      # a state, no estimate
        for missing in NEEDED:                                                         # an estimate without one of the four fields
            assert lib.sqair_set_estimate(h, C.byref(_est(without=(missing,))), T, B) == 0
            assert on() == -1 and "box, presence, obj_id and map_count" in _err(lib, h), missing
        assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
        for t in (1, 3, 0):      # another T
            assert on(t=t) == -1 and "T = {}".format(t) in _err(lib, h) and "T = 2" in _err(lib, h)
        assert on(b=B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        for bad in (0, -1, 17, 1 << 20):
            assert on(_score(G=bad)) == -1 and "must lie in 1..16" in _err(lib, h), bad
        for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
            assert on(_score(iou_min=bad)) == -1 and "iou_min must lie in (0, 1]" in _err(lib, h), bad
        for missing in _capi.SCORE_INPUTS:
            assert on(_score(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h) and missing in _err(lib, h), missing
        for ok in (1e-6, 0.5, 1.0):
            assert on(_score(iou_min=ok)) == 0
        for G in (1, 16):
            assert on(_score(G=G)) == 0
        for outs in ((), ("tp",), ("truth_match", "match_iou")):      # the per-frame outputs are optional
            assert on(_score(outputs=outs)) == 0, outs
        assert lib.sqair_set_score(h, None, 0, 0) == 0       # NULL: off


def test_a_pass_of_another_t_is_refused_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0
        assert lib.sqair_set_score(h, C.byref(_score()), 2, B) == 0
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            for T in (1, 3):
                assert fn(*_fwd_args(h, B, T=T)) == -1
                assert "T = 2" in _err(lib, h) and "T = {}".format(T) in _err(lib, h)


def test_the_estimate_or_the_state_going_off_takes_the_score_with_it():
    """The score can only be set while an estimate with the four fields is: after anything that switches it off, setting it again is
    refused until the estimate is back -- a NULL estimate, another T of the estimate, the state off and another B all switch it off."""
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        on = lambda T=2, b=B: lib.sqair_set_score(h, C.byref(_score()), T, b)
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0                     # the estimate off
        assert on() == -1 and "needs an estimate" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0
        assert lib.sqair_set_estimate(h, C.byref(_est(iou_min=0.3)), 2, B) == 0  # the same T again: the score stays
        assert lib.sqair_set_estimate(h, C.byref(_est()), 3, B) == 0          # another T: off; only the new T is taken
        assert on(2) == -1 and on(3) == 0
        assert lib.sqair_set_layers(h, C.byref(_capi.SqairLaneLayers(cover_min=0.5, match=0x9000)), 3, B) == 0   # beside the layers
        assert lib.sqair_set_layers(h, None, 0, 0) == 0 and on(3) == 0
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0            # the state off: the estimate and the score with it
        assert on(3) == -1 and "needs an estimate" in _err(lib, h)
        _state(lib, h, B)
        assert on(3) == -1 and "needs an estimate" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0
        _state(lib, h, B + 1)                                                 # another B
        assert on(2, B + 1) == -1 and "needs an estimate" in _err(lib, h)


def test_training_calls_never_run_the_score():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and lib.sqair_set_score(h, C.byref(_score()), 2, B) == 0
        assert lib.sqair_forward_train(*_fwd_args(h, B, T=2)) == -1 and "carried state" in _err(lib, h)


@pytest.mark.parametrize("path", LIBS)
def test_kernel_entry_point_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        good = dict(box=DUMMY, presence=DUMMY, obj_id=DUMMY, map_count=DUMMY, T=1, B=3)
        order = ("box", "presence", "obj_id", "map_count", "T", "B")
        call = lambda sc, **kw: lib.sqair_lane_score_test(h, *[dict(good, **kw)[k] for k in order], C.byref(sc) if sc is not None else None, DUMMY)
        assert lib.sqair_lane_score_test(None, *[good[k] for k in order], C.byref(_score()), DUMMY) == -1
        for kw in (dict(box=None), dict(presence=None), dict(obj_id=None), dict(map_count=None), dict(T=0), dict(T=65536), dict(B=0)):
            assert call(_score(), **kw) == -1 and "sqair_lane_score_test" in _err(lib, h), kw
        assert call(None) == -1
        for bad in (0.0, 1.5, float("nan")):
            assert call(_score(iou_min=bad)) == -1 and "iou_min" in _err(lib, h)
        for bad in (0, 17):
            assert call(_score(G=bad)) == -1 and "1..16" in _err(lib, h)
        for missing in _capi.SCORE_INPUTS:
            assert call(_score(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h)


def test_stream_argument_errors():
    """The score's arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    with pytest.raises(ValueError, match=r"^SqairStream: score is for a stream with estimate=True"):
        SqairStream(Core(), 2, score=True)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"^SqairStream: score_iou must lie in \(0, 1\]"):
            SqairStream(Core(), 2, estimate=True, score=True, score_iou=bad)
    for bad in (0, 17, -3, 2.5, True, "4"):
        with pytest.raises(ValueError, match=r"^SqairStream: score_truth must be an integer in \[1, 16\]"):
            SqairStream(Core(), 2, estimate=True, score=True, score_truth=bad)
