"""No GPU: the C-ABI of the object layers (include/sqair_hip.h: sqair_set_layers, sqair_lane_layers_test) -- exported and declared,
the binding mirrors the header's struct, the header's paragraph carries the semantics, every refusal is made before any HIP call
(dummy device pointers are enough), the layers go off with the estimate and the state -- and the argument errors of
SqairStream(estimate_layers=...)."""
import ctypes as C

import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, constant, err as _err, estimate as _est, fields as header_fields, fwd_args as _fwd_args, handle,
                            paragraph, phrases, prototype, set_state as _state, stated_once)


def _lay(cover_min=0.5, **kw):
    if not kw:
        kw = dict(match=0x5000, layer=0x6000, cover=0x7000, owner=0x8000)
    return _capi.SqairLaneLayers(cover_min=cover_min, **kw)


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, "sqair_set_layers") and hasattr(lib, "sqair_lane_layers_test") and lib.sqair_abi_version() == 2
    assert "sqair_set_layers" in _capi.EXPORTED_SYMBOLS and "sqair_lane_layers_test" in _capi.EXPORTED_SYMBOLS
    assert prototype("sqair_set_layers") == "int sqair_set_layers(SqairHandle* h, const SqairLaneLayers* lay, int T, int B)"
    assert prototype("sqair_lane_layers_test") == ("int sqair_lane_layers_test(SqairHandle* h, const float* glimpse, const float* where, "
                                                   "const float* presence, const float* lw, const float* log_w, float iou_min, int T, int B, "
                                                   "int K, const SqairLaneLayers* lay, void* stream)")
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    # the binding's struct mirrors the header's, field for field and in order
    fields = header_fields("SqairLaneLayers")
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairLaneLayers._fields_]
    assert [n for ty, n in fields if ty == "int32_t*"] == list(_capi.LAYERS_INT_FIELDS)
    assert [n for _, n in fields][1:] == list(_capi.LAYERS_FIELDS)
    assert _capi.layers_shapes(2, 3, 5, 4, (7, 9)) == dict(match=(2, 3, 5, 4), layer=(2, 3, 4, 7, 9), cover=(2, 3, 4, 7, 9), owner=(2, 3, 7, 9))


def test_the_header_states_the_semantics_once():
    doc = paragraph("object layers: per-object appearance", "typedef struct SqairLaneLayers")
    phrases(doc, ("k_lane_layers", "directly after k_lane_estimate", "BEFORE the SMC resampler", "exactly one kernel node more",
                  "Training passes never run it", "V(r, m) = p * (inverse spatial transformer of g)", "a glimpse of ones",
                  "sq_canvas_coord, sq_canvas_tap", "points 1, 2, 4 and 5", "iou_min and log_w", "match[t,b,k,j] (int32)",
                  "the estimate's support, summed in the same order", "index order", "no float atomics", "Absent j: zeros",
                  "a convex combination", "the first present j of maximal cover", "cover_min", "A NaN never wins", "Non-finite lanes",
                  "match and owner -1", "Coasted", "At K = 1", "sigmoid(-10 + 20 sum_j cover[j])", "owner needs no cover bound",
                  "Refused", "Out of scope"))
    stated_once("object layers: per-object appearance")


@pytest.mark.parametrize("path", LIBS)
def test_set_layers_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        B, T = 4, 2
        assert lib.sqair_set_layers(None, C.byref(_lay()), T, B) == -1
        assert lib.sqair_set_layers(h, C.byref(_lay()), T, B) == -1 and "sqair_set_estimate" in _err(lib, h)       # no state, no estimate
        _state(lib, h, B)
        assert lib.sqair_set_layers(h, C.byref(_lay()), T, B) == -1 and "needs an estimate" in _err(lib, h)        # a state, no estimate
        assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == 0
        for t in (1, 3, 0):      # another T
            assert lib.sqair_set_layers(h, C.byref(_lay()), t, B) == -1
            assert "T = {}".format(t) in _err(lib, h) and "T = 2" in _err(lib, h)
        assert lib.sqair_set_layers(h, C.byref(_lay()), T, B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
            assert lib.sqair_set_layers(h, C.byref(_lay(cover_min=bad)), T, B) == -1 and "cover_min must lie in (0, 1]" in _err(lib, h), bad
        none = _capi.SqairLaneLayers(cover_min=0.5)
        assert lib.sqair_set_layers(h, C.byref(none), T, B) == -1 and "at least one of match, layer, cover and owner" in _err(lib, h)
        for ok in (1e-6, 0.5, 1.0):
            assert lib.sqair_set_layers(h, C.byref(_lay(cover_min=ok)), T, B) == 0
        for one in ("match", "layer", "cover", "owner"):      # every pointer optional
            assert lib.sqair_set_layers(h, C.byref(_lay(**{one: 0x5000})), T, B) == 0, one
        assert lib.sqair_set_layers(h, None, 0, 0) == 0       # NULL: off


def test_a_pass_of_another_t_is_refused_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0
        assert lib.sqair_set_layers(h, C.byref(_lay()), 2, B) == 0
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            for T in (1, 3):
                assert fn(*_fwd_args(h, B, T=T)) == -1
                assert "T = 2" in _err(lib, h) and "T = {}".format(T) in _err(lib, h)


def test_the_estimate_or_the_state_going_off_takes_the_layers_with_it():
    """The layers can only be set while an estimate is: after anything that switches them off, setting them again is refused until
    the estimate is back -- and a NULL estimate, another T of the estimate, the state off and another B all switch them off."""
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        on = lambda T=2, b=B: lib.sqair_set_layers(h, C.byref(_lay()), T, b)
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0                     # the estimate off
        assert on() == -1 and "needs an estimate" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0
        assert lib.sqair_set_estimate(h, C.byref(_est(iou_min=0.3)), 2, B) == 0  # the same T again: the layers stay, at the new iou_min
        assert lib.sqair_set_estimate(h, C.byref(_est()), 3, B) == 0          # another T: off; only the new T is taken
        assert on(2) == -1 and on(3) == 0
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0            # the state off: the estimate and the layers with it
        assert on(3) == -1 and "needs an estimate" in _err(lib, h)
        _state(lib, h, B)
        assert on(3) == -1 and "needs an estimate" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and on() == 0
        _state(lib, h, B + 1)                                                 # another B
        assert on(2, B + 1) == -1 and "needs an estimate" in _err(lib, h)


def test_training_calls_never_run_the_layers():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0 and lib.sqair_set_layers(h, C.byref(_lay()), 2, B) == 0
        assert lib.sqair_forward_train(*_fwd_args(h, B, T=2)) == -1 and "carried state" in _err(lib, h)


@pytest.mark.parametrize("path", LIBS)
def test_kernel_entry_point_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        good = dict(glimpse=DUMMY, where=DUMMY, presence=DUMMY, lw=DUMMY, log_w=DUMMY, iou_min=0.5, T=1, B=3, K=5)
        order = ("glimpse", "where", "presence", "lw", "log_w", "iou_min", "T", "B", "K")
        call = lambda lay, **kw: lib.sqair_lane_layers_test(h, *[dict(good, **kw)[k] for k in order],
                                                            C.byref(lay) if lay is not None else None, DUMMY)
        assert lib.sqair_lane_layers_test(None, *[good[k] for k in order], C.byref(_lay()), DUMMY) == -1
        for kw in (dict(glimpse=None), dict(where=None), dict(presence=None), dict(lw=None), dict(T=0), dict(T=65536), dict(B=0), dict(K=0),
                   dict(K=257), dict(B=1 << 30, K=256)):
            assert call(_lay(), **kw) == -1 and "sqair_lane_layers_test" in _err(lib, h), kw
        assert call(None) == -1
        for bad in (0.0, 1.5, float("nan")):
            assert call(_lay(), iou_min=bad) == -1 and "iou_min" in _err(lib, h)
            assert call(_lay(cover_min=bad)) == -1 and "cover_min" in _err(lib, h)
        assert call(_capi.SqairLaneLayers(cover_min=0.5)) == -1 and "at least one of" in _err(lib, h)


def test_stream_argument_errors():
    """The layers' arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    with pytest.raises(ValueError, match=r"^SqairStream: estimate_layers is for a stream with estimate=True"):
        SqairStream(Core(), 2, estimate_layers=True)
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"^SqairStream: layers_cover_min must lie in \(0, 1\]"):
            SqairStream(Core(), 2, estimate=True, estimate_layers=True, layers_cover_min=bad)
