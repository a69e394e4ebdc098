"""No GPU: the C-ABI of per-frame matching (include/sqair_hip.h: sqair_set_lane_match) -- exported and declared, the ABI version
unchanged, the header's paragraph carries the semantics beside the three paragraphs that used to call it out of scope, every refusal
is made before any HIP call, the setting is a plain one that no registration touches -- and the argument errors of
SqairStream(score_match=..., identity_match=...) and of forecast / tracks(link_match=...)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (LIBS, ROOT, constant, err as _err, estimate, handle, paragraph, phrases, prototype, score, set_state,
                            stated_once)


def test_the_symbol_is_exported_and_declared_and_the_abi_is_unchanged():
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, "sqair_set_lane_match") and lib.sqair_abi_version() == 2
    assert "sqair_set_lane_match" in _capi.EXPORTED_SYMBOLS
    assert prototype("sqair_set_lane_match") == "int sqair_set_lane_match(SqairHandle* h, int score, int identity, int traj_link)"
    fn = _capi.lib().sqair_set_lane_match
    assert fn.restype is C.c_int and list(fn.argtypes) == [C.c_void_p, C.c_int, C.c_int, C.c_int]
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    # no struct changes: the three public structs are the sizes they were
    assert C.sizeof(_capi.SqairLaneScore) == 8 + 8 * 12 and C.sizeof(_capi.SqairLaneIdentity) == 24 + 8 * 11
    # the device function stands beside the other two
    lane_h = open(os.path.join(ROOT, "sqair_amd", "csrc", "sqair_lane.h")).read()
    for name in ("sq_assign_keep_greedy", "sq_assign_optimal_i32", "sq_assign_keep_optimal"):
        assert "__device__ __forceinline__" in lane_h and re.search(r"\b{}\(".format(name), lane_h), name
    assert "2^24 < 2^25" in lane_h and "below 2^30" in lane_h.replace("< 2^30", "below 2^30")


def test_the_header_states_the_semantics_once():
    doc = paragraph("per-frame matching: keep + optimal where the lane block matches keep + greedy", "int sqair_set_lane_match(")
    phrases(doc, ("CLEAR-MOT", "[[0.60, 0.54], [0.54, 0.08]]", "tp 1, fn 1, fp 1", "0 = keep + greedy (the default", "1 = keep + optimal",
                  "re-identification, births and ageing are untouched", "the link of sqair_lane_traj_score",
                  "A kept pair is never given up, even where that costs a pair", "keeps idsw comparable",
                  "maximises first the NUMBER of pairs, then the sum of q(g, j)", "q = __float2int_rn(IoU * 1048576.0f)", "units of 2^-20",
                  "2^25 + q", "-1 for every other pair", "2^24 < 2^25", "below 2^30", "sq_assign_optimal_i32", "on the table as it stands",
                  "a pair of weight -1 is never taken", "sq_assign_keep_optimal", "optimal assignments tie",
                  "whatever sq_assign_optimal_i32 returns", "the same bits eager, graph-replayed and in split passes",
                  "not restated as a rule", "matched and frag", "follow the score's mode", "it needs no registration",
                  "a captured graph freezes it, as it freezes pointers",
                  "sqair_lane_score_test, sqair_lane_identity_test and sqair_lane_idf_test",
                  "The node count of a pass does not depend on it", "before any HIP call", "a value other than 0 or 1",
                  "optimal re-identification", "HOTA"))
    stated_once("per-frame matching: keep + optimal where the lane block matches keep + greedy")
    # the three paragraphs keep their sentences and point here
    score_doc = paragraph("stream scoring: CLEAR-MOT events", "typedef struct SqairLaneScore")
    ident = paragraph("lane identities: stable per-lane track ids", "typedef struct SqairLaneIdentity")
    traj = paragraph("trajectory scoring: a lane forecast or a lane track table", "#define SQAIR_TRAJ_COUNTS")
    idf = paragraph("IDF1 scoring: does an identity stay on an object", "typedef struct SqairLaneIdf")
    for para in (score_doc, ident, traj):
        assert "Out of scope" in para and "optimal (Hungarian) assignment" in para and "sqair_set_lane_match's, below" in para
    assert "are sqair_set_idf's, below" in score_doc and "the device function is shaped for it" in idf and "sqair_set_lane_match" in idf
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):      # they point to the header, they do not restate it
        text = open(os.path.join(ROOT, name)).read()
        assert "sqair_set_lane_match" in text, name
        assert "__float2int_rn" not in text or name == "DESIGN.md", name


@pytest.mark.parametrize("path", LIBS)
def test_refusals_before_any_hip_call_and_a_setting_no_registration_touches(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        assert lib.sqair_set_lane_match(None, 0, 0, 0) == -1 and lib.sqair_set_lane_match(None, 1, 1, 1) == -1
        for bad in (2, -1, 7, 1 << 20):
            for pos, name in enumerate(("score", "identity", "traj_link")):
                args = [1, 1, 1]
                args[pos] = bad
                assert lib.sqair_set_lane_match(h, 0, 0, 0) == 0
                assert lib.sqair_set_lane_match(h, *args) == -1
                assert "sqair_set_lane_match: {} = {}".format(name, bad) in _err(lib, h) and "must be 0 (keep + greedy) or 1 (keep + optimal)" in _err(lib, h)
                # nothing was changed: the kernel-level entry of the score still refuses for its own reasons only, and a valid call passes
        for args in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
            assert lib.sqair_set_lane_match(h, *args) == 0, args
        # the setting survives every registration going on and off (none of these calls touches the device)
        B, T = 4, 2
        assert lib.sqair_set_lane_match(h, 1, 1, 1) == 0
        assert lib.sqair_set_score(h, None, 0, 0) == 0 and lib.sqair_set_identity(h, None, 0, 0) == 0 and lib.sqair_set_idf(h, None, 0, 0) == 0
        set_state(lib, h, B)
        est = estimate(fields=("box", "presence", "obj_id", "map_count"))
        assert lib.sqair_set_estimate(h, C.byref(est), T, B) == 0
        assert lib.sqair_set_score(h, C.byref(score(outputs=())), T, B) == 0 and lib.sqair_set_score(h, None, 0, 0) == 0
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0 and lib.sqair_set_state(h, None, None, None, 0, 0) == 0
        # ... which the stand-alone link shows: with traj_link still 1 a refusal of its own comes first, as it always did
        assert lib.sqair_lane_traj_score(h, None, None, None, 1, 1, None) == -1 and "must not be NULL" in _err(lib, h)
        assert lib.sqair_set_lane_match(h, 0, 0, 0) == 0


def test_the_python_arguments_and_their_errors():
    sig = inspect.signature(SqairStream.__init__).parameters
    assert sig["score_match"].default == "greedy" and sig["identity_match"].default == "greedy"
    assert inspect.signature(SqairStream.forecast).parameters["link_match"].default == "greedy"
    assert inspect.signature(SqairStream.tracks).parameters["link_match"].default == "greedy"

    class Core(object):      # (the keyword checks run before the stream touches its core)
        class cfg(object):
            sample_from_prior = False
    who = r"^SqairStream: "
    with pytest.raises(ValueError, match=who + "score_match must be 'greedy' or 'optimal'"):
        SqairStream(Core(), 2, estimate=True, score=True, score_match="hungarian")
    with pytest.raises(ValueError, match=who + "identity_match must be 'greedy' or 'optimal'"):
        SqairStream(Core(), 2, estimate=True, identity=True, identity_match=1)
    with pytest.raises(ValueError, match=who + "score_match='optimal' is for a stream with score=True"):
        SqairStream(Core(), 2, estimate=True, score_match="optimal")
    with pytest.raises(ValueError, match=who + "identity_match='optimal' is for a stream with identity=True"):
        SqairStream(Core(), 2, estimate=True, score=True, score_match="optimal", identity_match="optimal")
    # link_match: a call with truth
    from sqair_amd.lane import LaneAnswers, TrajScores
    la = LaneAnswers("SqairStream", False, 0.5, False, False, 0.5, False, 0.5, None, False, 0.3, None, 10, 4.0, float("inf"), True, "row")
    assert (la.score_match, la.identity_match) == (0, 0)
    ts = TrajScores(None, 3, la)
    for fn in ("SqairStream.forecast: ", "SqairStream.tracks: "):
        with pytest.raises(ValueError, match="^" + re.escape(fn) + "link_match must be 'greedy' or 'optimal'"):
            ts.check_truth(fn, None, True, 4, True, False, 0.5, "best")
        with pytest.raises(ValueError, match="^" + re.escape(fn) + "link_match='optimal' is for a call with truth"):
            ts.check_truth(fn, None, True, 4, True, False, 0.5, "optimal")
        assert ts.check_truth(fn, None, True, 4, True, False, 0.5, "greedy") is None
    truth = dict(box=np.zeros((4, 3, 2, 4), np.float32), present=np.ones((4, 3, 2), np.int32))
    got = ts.check_truth("SqairStream.tracks: ", truth, True, 4, True, False, 0.5, "optimal")
    assert got["G"] == 2 and "match" not in got       # (the checked truth is the ABI's names; the mode travels beside it)
