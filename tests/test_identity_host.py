"""No GPU: the C-ABI of lane identities (include/sqair_hip.h: sqair_set_identity, sqair_lane_identity_test, sqair_set_score_ids) --
exported and declared, the binding mirrors the header's struct, the header's paragraph carries the semantics, every refusal is made
before any HIP call (dummy device pointers are enough), the identity goes off with the estimate and the state and takes score_ids with
it -- and the argument errors of SqairStream(identity=...)."""
import ctypes as C
import functools
import os

import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, constant, dummy, err as _err, estimate, fields as header_fields, fwd_args as _fwd_args,
                            handle, paragraph, phrases, prototype, score, set_state as _state, stated_once)

NEEDED = ("box", "presence", "obj_id")      # (best_row is the estimate's own requirement)
REQUIRED = tuple(n for n in _capi.IDENT_MEMORY if n != "trk_what") + ("lane_id",)
INF = float("inf")
N = 3
_est = functools.partial(estimate, fields=NEEDED + ("map_count", "what"))
_score = functools.partial(score, outputs=())


def _ident(iou_min=0.3, reid_dist=4.0, reid_what=INF, M=6, max_age=10, without=(), outputs=_capi.IDENT_FIELDS):
    idt = dummy(_capi.SqairLaneIdentity, 0x5000, _capi.IDENT_MEMORY, without, iou_min=iou_min, reid_dist=reid_dist, reid_what=reid_what,
                M=M, max_age=max_age)
    for i, n in enumerate(outputs):
        setattr(idt, n, None if n in without else 0x7000 + 0x100 * i)
    return idt


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    names = ("sqair_set_identity", "sqair_lane_identity_test", "sqair_set_score_ids")
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert all(hasattr(lib, n) for n in names) and lib.sqair_abi_version() == 2
    assert all(n in _capi.EXPORTED_SYMBOLS for n in names)
    assert prototype("sqair_set_identity") == "int sqair_set_identity(SqairHandle* h, const SqairLaneIdentity* id, int T, int B)"
    assert prototype("sqair_lane_identity_test") == ("int sqair_lane_identity_test(SqairHandle* h, const float* box, const float* presence, "
                                                     "const float* obj_id, const float* what, const int32_t* best_row, int T, int B, "
                                                     "const SqairLaneIdentity* id, void* stream)")
    assert prototype("sqair_set_score_ids") == "int sqair_set_score_ids(SqairHandle* h, int lane_ids)"
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    assert constant("SQAIR_IDENT_MAX_TRACKS") == _capi.IDENT_MAX_TRACKS == 16
    assert constant("SQAIR_IDENT_COUNTS") == len(_capi.IDENT_COUNTS) == 8
    # the binding's struct mirrors the header's, field for field and in order
    fields = header_fields("SqairLaneIdentity")
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairLaneIdentity._fields_]
    assert [n for _, n in fields] == [n for n, _ in _capi.IDENT_SCALARS] + list(_capi.IDENT_MEMORY) + list(_capi.IDENT_FIELDS)
    assert [n for _, n in fields][:5] == ["iou_min", "reid_dist", "reid_what", "M", "max_age"]
    types = {n: ty for ty, n in fields}
    assert [types[n] for n, _ in _capi.IDENT_SCALARS] == ["float", "float", "float", "int32_t", "int32_t"]
    assert [n for ty, n in fields if ty == "float*"] == ["trk_box", "trk_what"] and types["counts"] == "int64_t*"
    assert [n for ty, n in fields if ty == "int32_t*"] == ["trk_id", "trk_word", "trk_age", "trk_len", "next_id", "lane_id", "how", "track_len"]
    assert C.sizeof(_capi.SqairLaneIdentity) == 24 + 8 * 11 and _capi.SqairLaneIdentity.trk_id.offset == 24
    assert _capi.SqairLaneIdentity.M.offset == 12 and _capi.SqairLaneIdentity.max_age.offset == 16
    assert _capi.identity_shapes(2, 3, 5) == dict(lane_id=(2, 3, 5), id_how=(2, 3, 5), track_len=(2, 3, 5))
    assert _capi.identity_memory_shapes(3, 6, 50) == dict(trk_id=(3, 6), trk_word=(3, 6), trk_age=(3, 6), trk_len=(3, 6), trk_box=(3, 6, 4),
                                                          trk_what=(3, 6, 50), next_id=(3,), counts=(3, 8))
    # the counters' order is the header's
    assert "counts [B,8] int64: frames, frames_invalid, objects (present slots seen), kept, bridged, reidentified, born" in paragraph()
    assert _capi.IDENT_COUNTS == ("frames", "frames_invalid", "objects", "kept", "bridged", "reidentified", "born", "ended")


def test_the_header_states_the_semantics_once():
    doc = paragraph("lane identities: stable per-lane track ids", "typedef struct SqairLaneIdentity")
    phrases(doc, ("k_lane_identity", "one workgroup per lane", "after k_lane_estimate (and after k_lane_layers if on)",
                  "BEFORE k_lane_score if on", "BEFORE the SMC resampler", "exactly one kernel node more", "unchanged bit for bit",
                  "Training passes never run it", "does not read the records again", "trk_id (-1 = free", "never read", "the obj_id WORD",
                  "next_id[b]", "Non-finite lane (best_row[t,b] == -1)", "frames_invalid += 1", "no ageing",
                  "sq_box_iou(trk_box[e], box[t,b,j])", "ONE call of sq_assign_keep_greedy", "keep_id[e] = trk_word[e]",
                  "col_id[j] = the obj_id word of slot j", "IoU >= iou_min", "ties to the smallest e, then the smallest j",
                  "a NaN never passes", "how = 1 (kept)", "how = 2 (bridged", "only when reid_dist > 0", "(y + 0.5 h, x + 0.5 w)",
                  "r = reid_dist * (trk_age[e] + 1)", "dc2 <= r * r", "dw <= reid_what", "fmaf(d, d, acc)", "/ n_what in fp32",
                  "A NaN never passes", "minimal dw", "minimal dc2", "ties to the smallest e", "how = 3 (re-identified)",
                  "Greedy in j on purpose", "trk_age = 0, trk_len += 1", "lane_id[t,b,j] = trk_id[e]", "track_len[t,b,j] = trk_len[e]",
                  "the first free entry", "largest trk_age", "evicted (ended += 1)", "M >= N guarantees", "next_id[b] += 1",
                  "how = 0 (born)", "exceeds max_age", "Coasted", "in place", "two passes of three frames leave the bits of one pass of six",
                  "an id is never reused within a lane", "how and track_len are optional", "Refused", "M outside N..16", "reid_dist negative",
                  "reid_what not in (0, +inf]", "max_age < 0", "any NaN among the scalars", "trk_what given while the estimate binds no what",
                  "a pass of another T", "switch the identity off", "sqair_set_score_ids(h, 1)",
                  "refused unless both the score and the identity are set", "puts it back to 0", "Out of scope",
                  "lane tracks and lane forecasts", "optimal (Hungarian) assignment", "a motion model", "identities across lanes",
                  "training passes"))
    stated_once("lane identities: stable per-lane track ids")
    for name in ("DESIGN.md", "README.md"):      # they point to the header, they do not restate it
        assert "sqair_set_identity" in open(os.path.join(ROOT, name)).read(), name


@pytest.mark.parametrize("path", LIBS)
def test_set_identity_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        B, T = 4, 2
        on = lambda idt=None, t=T, b=B: lib.sqair_set_identity(h, C.byref(idt or _ident()), t, b)
        assert lib.sqair_set_identity(None, C.byref(_ident()), T, B) == -1
        assert on() == -1 and "sqair_set_estimate" in _err(lib, h)                    # no state, no estimate
        _state(lib, h, B)
        assert on() == -1 and "needs an estimate" in _err(lib, h)                      # a state, no estimate
        for missing in NEEDED:                                                         # an estimate without one of the fields
            assert lib.sqair_set_estimate(h, C.byref(_est(without=(missing,))), T, B) == 0
            assert on() == -1 and "box, presence, obj_id and best_row" in _err(lib, h), missing
        assert lib.sqair_set_estimate(h, C.byref(_est(without=("what",))), T, B) == 0   # trk_what needs the estimate's what
        assert on() == -1 and "trk_what needs the estimate" in _err(lib, h)
        assert on(_ident(without=("trk_what",))) == 0
        assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
        for t in (1, 3, 0):      # another T
            assert on(t=t) == -1 and "T = {}".format(t) in _err(lib, h) and "T = 2" in _err(lib, h)
        assert on(b=B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        for bad in (N - 1, 0, -1, 17, 1 << 20):
            assert on(_ident(M=bad)) == -1 and "must lie in N = 3..16" in _err(lib, h), bad
        for bad in (0.0, -0.5, 1.0000001, float("nan"), INF):
            assert on(_ident(iou_min=bad)) == -1 and "iou_min must lie in (0, 1]" in _err(lib, h), bad
        for bad in (-1e-6, -INF, float("nan")):
            assert on(_ident(reid_dist=bad)) == -1 and "reid_dist must be >= 0" in _err(lib, h), bad
        for bad in (0.0, -1.0, -INF, float("nan")):
            assert on(_ident(reid_what=bad)) == -1 and "reid_what must lie in (0, +inf]" in _err(lib, h), bad
        for bad in (-1, -(1 << 20)):
            assert on(_ident(max_age=bad)) == -1 and "max_age must be >= 0" in _err(lib, h), bad
        for missing in REQUIRED:
            assert on(_ident(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h) and missing in _err(lib, h), missing
        for kw in (dict(iou_min=1e-6), dict(iou_min=1.0), dict(reid_dist=0.0), dict(reid_dist=INF), dict(reid_what=1e-6), dict(reid_what=INF),
                   dict(M=N), dict(M=16), dict(max_age=0), dict(max_age=1 << 20)):
            assert on(_ident(**kw)) == 0, kw
        for outs in (("lane_id",), ("lane_id", "how"), ("lane_id", "track_len")):      # how and track_len are optional
            assert on(_ident(outputs=outs)) == 0, outs
        assert lib.sqair_set_identity(h, None, 0, 0) == 0       # NULL: off


def test_a_pass_of_another_t_is_refused_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=N) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0
        assert lib.sqair_set_identity(h, C.byref(_ident()), 2, B) == 0
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            for T in (1, 3):
                assert fn(*_fwd_args(h, B, T=T)) == -1
                assert "T = 2" in _err(lib, h) and "T = {}".format(T) in _err(lib, h)
        assert lib.sqair_forward_train(*_fwd_args(h, B, T=2)) == -1 and "carried state" in _err(lib, h)   # training never runs it


def test_the_estimate_or_the_state_going_off_takes_the_identity_with_it():
    """The identity can only be set while an estimate with its fields is: after anything that switches it off, setting score_ids is
    refused (that needs the identity) until it is set again."""
    with handle(k_particles=2, n_steps_per_image=N) as (lib, h):
        B = 4
        on = lambda T=2, b=B, **kw: lib.sqair_set_identity(h, C.byref(_ident(**kw)), T, b)
        score = lambda T=2: lib.sqair_set_score(h, C.byref(_score()), T, B)
        ids = lambda v=1: lib.sqair_set_score_ids(h, v)
        is_on = lambda: ids(1) == 0      # (with a score set: score_ids is accepted exactly while the identity is on)
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0 and score() == 0 and is_on()
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0                     # the estimate off
        assert on() == -1 and "needs an estimate" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and score() == 0 and not is_on() and on() == 0 and is_on()
        assert lib.sqair_set_estimate(h, C.byref(_est(iou_min=0.3)), 2, B) == 0 and is_on()     # the same T again: the identity stays
        assert lib.sqair_set_estimate(h, C.byref(_est(without=("map_count",))), 2, B) == 0      # the score's field goes: the score off,
        assert not is_on() and score() == -1 and on() == 0                                      # the identity itself can stay
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and score() == 0 and is_on()
        for missing in NEEDED + ("what",):                                                      # one of its own fields goes: off
            assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0 and score() == 0 and is_on()
            assert lib.sqair_set_estimate(h, C.byref(_est(without=(missing,))), 2, B) == 0
            assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and score() == 0 and not is_on(), missing
        assert on(without=("trk_what",)) == 0                                                   # without trk_what, what may go
        assert lib.sqair_set_estimate(h, C.byref(_est(without=("what",))), 2, B) == 0 and score() == 0 and is_on()
        assert lib.sqair_set_estimate(h, C.byref(_est()), 3, B) == 0          # another T: off; only the new T is taken
        assert on(2) == -1 and on(3) == 0 and score(3) == 0 and is_on()
        assert lib.sqair_set_layers(h, C.byref(_capi.SqairLaneLayers(cover_min=0.5, match=0x9000)), 3, B) == 0   # beside the layers
        assert lib.sqair_set_layers(h, None, 0, 0) == 0 and is_on()
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0            # the state off: the estimate and the identity with it
        assert on(3) == -1 and "needs an estimate" in _err(lib, h)
        _state(lib, h, B)
        assert on(3) == -1 and "needs an estimate" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0
        _state(lib, h, B + 1)                                                 # another B
        assert on(2, B + 1) == -1 and "needs an estimate" in _err(lib, h)


def test_score_ids_needs_both_and_goes_back_with_either():
    with handle(k_particles=2, n_steps_per_image=N) as (lib, h):
        B, T = 4, 2
        ids = lambda v=1: lib.sqair_set_score_ids(h, v)
        refused = lambda: ids(1) == -1 and "needs both a score" in _err(lib, h)
        assert lib.sqair_set_score_ids(None, 1) == -1
        assert ids(0) == 0 and refused()                                       # nothing set: 0 is always accepted, 1 refused
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0 and refused()
        assert lib.sqair_set_score(h, C.byref(_score()), T, B) == 0 and refused()               # the score alone
        assert lib.sqair_set_score(h, None, 0, 0) == 0
        assert lib.sqair_set_identity(h, C.byref(_ident()), T, B) == 0 and refused()            # the identity alone
        assert lib.sqair_set_score(h, C.byref(_score()), T, B) == 0 and ids(1) == 0 and ids(0) == 0 and ids(1) == 0
        assert lib.sqair_set_identity(h, None, 0, 0) == 0 and refused()                         # the identity off
        assert lib.sqair_set_identity(h, C.byref(_ident()), T, B) == 0 and ids(1) == 0
        assert lib.sqair_set_score(h, None, 0, 0) == 0 and refused()                            # the score off


@pytest.mark.parametrize("path", LIBS)
def test_kernel_entry_point_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        good = dict(box=DUMMY, presence=DUMMY, obj_id=DUMMY, what=DUMMY, best_row=DUMMY, T=1, B=3)
        order = ("box", "presence", "obj_id", "what", "best_row", "T", "B")
        call = lambda idt, **kw: lib.sqair_lane_identity_test(h, *[dict(good, **kw)[k] for k in order],
                                                              C.byref(idt) if idt is not None else None, DUMMY)
        assert lib.sqair_lane_identity_test(None, *[good[k] for k in order], C.byref(_ident()), DUMMY) == -1
        for kw in (dict(box=None), dict(presence=None), dict(obj_id=None), dict(best_row=None), dict(T=0), dict(T=65536), dict(B=0)):
            assert call(_ident(), **kw) == -1 and "sqair_lane_identity_test" in _err(lib, h), kw
        assert call(None) == -1
        assert call(_ident(), what=None) == -1 and "trk_what needs what" in _err(lib, h)
        for bad in (0.0, 1.5, float("nan")):
            assert call(_ident(iou_min=bad)) == -1 and "iou_min" in _err(lib, h)
        for bad in (N - 1, 17):
            assert call(_ident(M=bad)) == -1 and "N = 3..16" in _err(lib, h)
        assert call(_ident(reid_dist=-1.0)) == -1 and call(_ident(reid_what=0.0)) == -1 and call(_ident(max_age=-1)) == -1
        assert call(_ident(reid_dist=float("nan"))) == -1 and call(_ident(reid_what=float("nan"))) == -1
        for missing in REQUIRED:
            assert call(_ident(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h)


def test_stream_argument_errors():
    """The identity's arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    with pytest.raises(ValueError, match=r"^SqairStream: identity is for a stream with estimate=True"):
        SqairStream(Core(), 2, identity=True)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"^SqairStream: identity_iou must lie in \(0, 1\]"):
            SqairStream(Core(), 2, estimate=True, identity=True, identity_iou=bad)
    for bad in (0, 17, -3, 2.5, True, "4"):
        with pytest.raises(ValueError, match=r"^SqairStream: identity_tracks must be an integer in \[n_steps_per_image, 16\]"):
            SqairStream(Core(), 2, estimate=True, identity=True, identity_tracks=bad)
    for bad in (-1, 2.5, True, "4", None):
        with pytest.raises(ValueError, match=r"^SqairStream: identity_max_age must be an integer >= 0"):
            SqairStream(Core(), 2, estimate=True, identity=True, identity_max_age=bad)
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError, match=r"^SqairStream: identity_reid_dist must be >= 0"):
            SqairStream(Core(), 2, estimate=True, identity=True, identity_reid_dist=bad)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match=r"^SqairStream: identity_reid_what must lie in \(0, \+inf\]"):
            SqairStream(Core(), 2, estimate=True, identity=True, identity_reid_what=bad)
    with pytest.raises(ValueError, match=r"^SqairStream: score_ids must be 'row' or 'lane'"):
        SqairStream(Core(), 2, estimate=True, identity=True, score=True, score_ids="both")
    for kw in (dict(identity=True), dict(score=True), dict()):
        with pytest.raises(ValueError, match=r"^SqairStream: score_ids='lane' is for a stream with score=True and identity=True"):
            SqairStream(Core(), 2, estimate=True, score_ids="lane", **kw)
