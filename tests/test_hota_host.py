"""No GPU: the C-ABI of HOTA scoring (include/sqair_hip.h: sqair_set_hota, sqair_lane_hota_test, sqair_lane_hota_solve) -- exported
and declared in all three libraries, the binding mirrors the header's struct, the header's paragraph carries the semantics and is
stated once, every refusal is made before any HIP call (dummy device pointers are enough), HOTA goes off with the score, the IDF and
matching paragraphs still hold their HOTA sentences -- and the argument errors of SqairStream(score_hota=...)."""
import ctypes as C
import functools
import os

import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, c_layout, constant, dummy, err as _err, estimate, fields as header_fields, fwd_args, handle,
                            paragraph, phrases, prototype, score as _score, set_state as _state, stated_once)

NEEDED = ("box", "presence", "obj_id", "map_count")
HOTA_POINTERS = _capi.HOTA_LOG + _capi.HOTA_TOTALS
_est = functools.partial(estimate, fields=NEEDED)
FIRST_WORDS = "HOTA scoring: detection, association and localisation in one figure"


def _hota(P=8, L=16, without=()):
    return dummy(_capi.SqairLaneHota, 0x9000, HOTA_POINTERS, without, P=P, L=L)


def _ready(lib, h, B=4, T=2, **score):
    _state(lib, h, B)
    assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
    assert lib.sqair_set_score(h, C.byref(_score(**score)), T, B) == 0


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    names = ("sqair_set_hota", "sqair_lane_hota_test", "sqair_lane_hota_solve")
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert all(hasattr(lib, n) for n in names) and lib.sqair_abi_version() == 2
    assert all(n in _capi.EXPORTED_SYMBOLS for n in names)
    assert prototype("sqair_set_hota") == "int sqair_set_hota(SqairHandle* h, const SqairLaneHota* hota, int T, int B)"
    assert prototype("sqair_lane_hota_test") == ("int sqair_lane_hota_test(SqairHandle* h, const float* box, const float* presence, "
                                                 "const float* ids, const int32_t* map_count, int T, int B, const SqairLaneScore* score, "
                                                 "const SqairLaneHota* hota, void* stream)")
    assert prototype("sqair_lane_hota_solve") == ("int sqair_lane_hota_solve(SqairHandle* h, const SqairLaneHota* hota, int G, int N, int B, "
                                                  "const int32_t* close, int64_t* open_i, double* open_f, int64_t* open_c, int32_t* match, "
                                                  "void* stream)")
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    assert constant("SQAIR_HOTA_ALPHAS") == _capi.HOTA_ALPHAS == 19
    assert constant("SQAIR_HOTA_MAX_IDS") == _capi.HOTA_MAX_IDS == 64
    assert constant("SQAIR_HOTA_MAX_FRAMES") == _capi.HOTA_MAX_FRAMES == 4096
    # the binding's struct mirrors the header's, field for field and in order
    fields = header_fields("SqairLaneHota")
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairLaneHota._fields_] == ["P", "L"] + list(HOTA_POINTERS)
    assert HOTA_POINTERS == ("col_id", "log_q", "log_col", "log_row", "frames", "dropped_frames", "work", "totals_i", "totals_f", "totals_c")
    assert [ty for ty, _ in fields] == ["int32_t"] * 2 + ["int32_t*"] * 7 + ["int64_t*", "double*", "int64_t*"]
    assert C.sizeof(_capi.SqairLaneHota) == 8 + 8 * 10
    assert _capi.hota_shapes(3, 4, 5, 6, 7) == dict(col_id=(3, 6), log_q=(3, 7, 4, 5), log_col=(3, 7, 5), log_row=(3, 7), frames=(3,),
                                                   dropped_frames=(3,), work=(3, 4, 6, 20), totals_i=(3, 19, 4), totals_f=(3, 19, 3),
                                                   totals_c=(3, 4))
    assert _capi.hota_solve_shapes(3, 4, 7) == dict(open_i=(3, 19, 4), open_f=(3, 19, 3), open_c=(3, 4), match=(3, 7, 4), close=(3,))
    # the totals' orders are the header's
    doc = paragraph()
    phrases(doc, ("totals_i [B,19,4] int64 = (tp, fn, fp, loc)", "totals_f [B,19,3] double = (ass, assre, asspr)",
                  "totals_c [B,4] int64 = (clips, frames, dropped_frames, overflow_ids"))
    assert (_capi.HOTA_INT, _capi.HOTA_FLOAT, _capi.HOTA_CLIP) == (("tp", "fn", "fp", "loc"), ("ass", "assre", "asspr"),
                                                                    ("clips", "frames", "dropped_frames", "overflow_ids"))


def test_the_struct_has_the_compilers_size(tmp_path):
    """sizeof and the offsets in C are what ctypes lays out."""
    names = ("P", "L", "col_id", "work", "totals_f", "totals_c")
    got = c_layout(tmp_path, dict(SqairLaneHota=names))
    assert got["SqairLaneHota"] == (C.sizeof(_capi.SqairLaneHota), [getattr(_capi.SqairLaneHota, n).offset for n in names])


def test_the_header_states_the_semantics_once():
    doc = paragraph(FIRST_WORDS, "typedef struct SqairLaneHota")
    phrases(doc, ("k_lane_hota", "one workgroup per lane", "after k_lane_score (and after k_lane_idf when that is on) and BEFORE the SMC resampler",
                  "exactly one kernel node more", "unchanged bit for bit",
                  "Training passes, and a capture's eager pre-pass without effects, never run it", "k_lane_hota_solve", "integer arithmetic",
                  "exactly the IDF's points 1 and 3", "truth_valid != 0 and map_count != -1", "the IDF's rule 3a", "P in 1..64",
                  "with or without an IDF", "iou_min and truth_match are NOT read", "L in 1..4096", "adds 1 to dropped_frames[b] and touches nothing else",
                  "q = __float2int_rn(IoU * 1048576.0f)", "sq_box_iou", "KEYED present object", "-1 for every other pair",
                  "-1: j is absent, -2: j is present but unkeyed", "bit g is set when truth g is present", "stale log words are never read",
                  "totals_c.overflow_ids, at once", "R_g = sum_j q", "C_j = sum_g q", "n(g,j) = (q * 2^20) / (R_g + C_j - q) in int64, truncating",
                  "0 when the denominator is 0", "pot[g, col(j)] += n", "extra += 1 for each unkeyed j",
                  "gas[g,p] = (pot * 2^20) / ((row_frames[g] + col_frames[p]) * 2^20 - pot)", "global_alignment_score",
                  "ONE assignment per record, not one per threshold", "w[g,j] = (gas[g, col(j)] * q[g,j]) >> 15", "w <= 2^25", "below 2^30",
                  "sq_assign_optimal_i32", "whatever that function returns", "not restated as a rule", "A_i = ceil(i * 2^20 / 20)", "A_10 = 2^19",
                  "tp_i += 1, loc_i += q and mc_i[g, col(j)] += 1", "match [B,L,G]", "fn_i = sum_g row_frames - tp_i",
                  "fp_i = sum_p col_frames + extra - tp_i", "ass_i = sum mc^2 / (row_frames[g] + col_frames[p] - mc)",
                  "assre_i = sum mc^2 / row_frames[g]", "asspr_i = sum mc^2 / col_frames[p]", "in a fixed order", "integer atomics",
                  "frees the lane", "AssA = ass / tp is weighted by TP", "DetA = tp / (tp + fn + fp)", "HOTA_a = sqrt(DetA AssA)",
                  "is refused (return -1", "no score set", "P outside 1..64", "L outside 1..4096", "HOTA goes off with the score", "another G",
                  "Out of scope", "a tie rule", "clips longer than L frames"))
    stated_once(FIRST_WORDS)
    assert paragraph().count("global_alignment_score") == 1 and paragraph().count("A_i = ceil(") == 1
    for name in ("DESIGN.md", "README.md"):      # they point to the header, they do not restate it
        text = open(os.path.join(ROOT, name)).read()
        assert "sqair_set_hota" in text and "global_alignment_score" not in text, name
    # the places that recorded the gap still say so, and point here now
    idf = paragraph("IDF1 scoring: does an identity stay on an object", "typedef struct SqairLaneIdf")
    assert "identities other than the slot; HOTA (sqair_set_hota, below); IDF1 per particle row" in idf
    match = paragraph("per-frame matching: keep + optimal", "int sqair_set_lane_match")
    assert "particle row; HOTA (sqair_set_hota, above); training passes." in match and "Not offered" in match
    lane_h = open(os.path.join(ROOT, "sqair_amd", "csrc", "sqair_lane.h")).read()
    assert "sq_lane_id_column" in lane_h


@pytest.mark.parametrize("path", LIBS)
def test_set_hota_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        B, T = 4, 2
        on = lambda hota=None, t=T, b=B: lib.sqair_set_hota(h, C.byref(hota or _hota()), t, b)
        assert lib.sqair_set_hota(None, C.byref(_hota()), T, B) == -1
        assert on() == -1 and "needs a score" in _err(lib, h)                          # no state, no estimate, no score
        _state(lib, h, B)
        assert on() == -1 and "needs a score" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
        assert on() == -1 and "needs a score" in _err(lib, h)                          # an estimate, no score
        assert lib.sqair_set_score(h, C.byref(_score(outputs=("tp",))), T, B) == 0     # truth_match is not needed
        assert on() == 0
        for t in (1, 3, 0):      # another T
            assert on(t=t) == -1 and "T = {}".format(t) in _err(lib, h) and "T = 2" in _err(lib, h)
        assert on(b=B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        for bad in (0, -1, 65, 1 << 20):
            assert on(_hota(P=bad)) == -1 and "P = {}".format(bad) in _err(lib, h) and "must lie in 1..64" in _err(lib, h), bad
        for bad in (0, -1, 4097, 1 << 20):
            assert on(_hota(L=bad)) == -1 and "L = {}".format(bad) in _err(lib, h) and "must lie in 1..4096" in _err(lib, h), bad
        for missing in HOTA_POINTERS:
            assert on(_hota(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h) and missing in _err(lib, h), missing
        for P, L in ((1, 1), (32, 256), (64, 4096)):
            assert on(_hota(P=P, L=L)) == 0
        assert lib.sqair_set_hota(h, None, 0, 0) == 0       # NULL: off


def test_the_score_going_off_takes_hota_with_it():
    """What switches HOTA off cannot be seen from outside but for the node it launches (tests/test_hota_stream.py counts those);
    here: after everything that switches the score off, setting HOTA again is refused until the score is back."""
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        on = lambda T=2, b=B: lib.sqair_set_hota(h, C.byref(_hota()), T, b)
        _ready(lib, h, B)
        assert on() == 0
        assert lib.sqair_set_score(h, None, 0, 0) == 0                          # the score off
        assert on() == -1 and "needs a score" in _err(lib, h)
        assert lib.sqair_set_score(h, C.byref(_score()), 2, B) == 0 and on() == 0
        assert lib.sqair_set_score(h, C.byref(_score(G=5)), 2, B) == 0 and on() == 0  # another G: off, and on again for the new one
        assert lib.sqair_set_idf(h, None, 0, 0) == 0 and on() == 0                    # with or without an IDF
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0                       # the estimate off: the score and HOTA with it
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


def test_training_calls_never_run_hota():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _ready(lib, h, B)
        assert lib.sqair_set_hota(h, C.byref(_hota()), 2, B) == 0
        assert lib.sqair_forward_train(*fwd_args(h, B, T=2)) == -1
        assert "carried state" in _err(lib, h)


@pytest.mark.parametrize("path", LIBS)
def test_kernel_entry_point_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        good = dict(box=DUMMY, presence=DUMMY, ids=DUMMY, map_count=DUMMY, T=1, B=3)
        order = ("box", "presence", "ids", "map_count", "T", "B")
        ref = lambda x: C.byref(x) if x is not None else None
        call = lambda sc, hota, **kw: lib.sqair_lane_hota_test(h, *[dict(good, **kw)[k] for k in order], ref(sc), ref(hota), DUMMY)
        assert lib.sqair_lane_hota_test(None, *[good[k] for k in order], C.byref(_score()), C.byref(_hota()), DUMMY) == -1
        for kw in (dict(box=None), dict(presence=None), dict(ids=None), dict(map_count=None), dict(T=0), dict(T=65536), dict(B=0)):
            assert call(_score(), _hota(), **kw) == -1 and "sqair_lane_hota_test" in _err(lib, h), kw
        assert call(None, _hota()) == -1 and call(_score(), None) == -1
        for bad in (0, 17):
            assert call(_score(G=bad), _hota()) == -1 and "1..16" in _err(lib, h)
        for missing in ("truth_box", "truth_present", "truth_valid"):
            assert call(_score(without=(missing,)), _hota()) == -1 and "must not be NULL" in _err(lib, h)
        for bad in (0, 65):
            assert call(_score(), _hota(P=bad)) == -1 and "1..64" in _err(lib, h)
        for bad in (0, 4097):
            assert call(_score(), _hota(L=bad)) == -1 and "1..4096" in _err(lib, h)
        for missing in HOTA_POINTERS:
            assert call(_score(), _hota(without=(missing,))) == -1 and missing in _err(lib, h)
        # the solve
        solve = lambda hota, G=4, N=3, B=3: lib.sqair_lane_hota_solve(h, ref(hota), G, N, B, None, None, None, None, None, DUMMY)
        assert lib.sqair_lane_hota_solve(None, C.byref(_hota()), 4, 3, 3, None, None, None, None, None, DUMMY) == -1
        assert solve(None) == -1 and "sqair_lane_hota_solve" in _err(lib, h)
        for bad in (0, 17):
            assert solve(_hota(), G=bad) == -1 and "1..16" in _err(lib, h)
            assert solve(_hota(), N=bad) == -1 and "N = {}".format(bad) in _err(lib, h)
        assert solve(_hota(), B=0) == -1 and "B = 0" in _err(lib, h)
        for bad in (0, 65):
            assert solve(_hota(P=bad)) == -1 and "1..64" in _err(lib, h)
        for bad in (0, 4097):
            assert solve(_hota(L=bad)) == -1 and "1..4096" in _err(lib, h)
        for missing in HOTA_POINTERS:
            assert solve(_hota(without=(missing,))) == -1 and missing in _err(lib, h)


def test_stream_argument_errors():
    """HOTA's arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    with pytest.raises(ValueError, match=r"^SqairStream: score_hota is for a stream with score=True"):
        SqairStream(Core(), 2, estimate=True, score_hota=True)
    with pytest.raises(ValueError, match=r"^SqairStream: score is for a stream with estimate=True"):
        SqairStream(Core(), 2, score=True, score_hota=True)
    for bad in (0, 65, -3, 2.5, True, "4", None):
        with pytest.raises(ValueError, match=r"^SqairStream: score_hota_ids must be an integer in \[1, 64\]"):
            SqairStream(Core(), 2, estimate=True, score=True, score_hota=True, score_hota_ids=bad)
    for bad in (0, 4097, -3, 2.5, True, "4", None):
        with pytest.raises(ValueError, match=r"^SqairStream: score_hota_frames must be an integer in \[1, 4096\]"):
            SqairStream(Core(), 2, estimate=True, score=True, score_hota=True, score_hota_frames=bad)
