"""No GPU: the C-ABI of the lane estimate (include/sqair_hip.h: sqair_set_estimate, sqair_lane_estimate_test) -- exported and
declared, the header's paragraph carries the semantics, every refusal is made before any HIP call (dummy device pointers are
enough), the estimate goes off with the state -- and the argument errors of SqairStream(estimate=...)."""
import ctypes as C

import pytest

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, constant, err as _err, estimate as _est, fields as header_fields, fwd_args as _fwd_args, handle,
                            paragraph, phrases, prototype, set_state as _state, smc as _smc, stated_once)


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, "sqair_set_estimate") and hasattr(lib, "sqair_lane_estimate_test") and lib.sqair_abi_version() == 2
    assert "sqair_set_estimate" in _capi.EXPORTED_SYMBOLS and "sqair_lane_estimate_test" in _capi.EXPORTED_SYMBOLS
    assert prototype("sqair_set_estimate") == "int sqair_set_estimate(SqairHandle* h, const SqairLaneEstimate* est, int T, int B)"
    assert prototype("sqair_lane_estimate_test") == ("int sqair_lane_estimate_test(SqairHandle* h, const float* where, const float* presence, "
                                                     "const float* obj_id, const float* what, const float* canvas, const float* lw, int T, "
                                                     "int B, int K, const SqairLaneEstimate* est, void* stream)")
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    # the binding's struct mirrors the header's, field for field and in order
    fields = header_fields("SqairLaneEstimate")
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairLaneEstimate._fields_]
    assert [n for ty, n in fields if ty == "int32_t*"] == list(_capi.ESTIMATE_INT_FIELDS)
    assert [n for _, n in fields][2:] == list(_capi.ESTIMATE_FIELDS)


def test_the_header_states_the_semantics_once():
    doc = paragraph("lane estimates: one answer per lane", "typedef struct SqairLaneEstimate")
    phrases(doc, ("k_lane_estimate", "BEFORE the", "exactly one kernel node more", "Training passes never run it",
                  "in frame order, in fp32", "index order", "bit for bit", "NULL means zeros", "the first k of maximal a_k",
                  "count_prob[t,b,c] = sum_k w_k [n_k = c]", "the first c of maximal count_prob",
                  "stn_to_pixel_coords(to_coords(where), (H, W))", "modules.py:221-262", "SPATIAL association", "not by id",
                  "the first present slot of row k with maximal IoU", "0 when the union is not positive", "iou_min", "NOT one-to-one",
                  "mean_canvas[t,b] = sum_k w_k canvas[t, r]", "out->canvas", "Non-finite lanes", "best_row = map_count = -1", "zero objects",
                  "Coasted", "Refused"))
    stated_once("lane estimates: one answer per lane")


def test_set_estimate_refusals_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        assert lib.sqair_set_estimate(None, C.byref(_est()), 1, B) == -1
        assert lib.sqair_set_estimate(h, C.byref(_est()), 1, B) == -1 and "carried state" in _err(lib, h)      # no state set
        _state(lib, h, B)
        for T in (0, -2):
            assert lib.sqair_set_estimate(h, C.byref(_est()), T, B) == -1 and "T must be >= 1" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 1, B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
            assert lib.sqair_set_estimate(h, C.byref(_est(iou_min=bad)), 1, B) == -1 and "iou_min must lie in (0, 1]" in _err(lib, h), bad
        assert lib.sqair_set_estimate(h, C.byref(_est(best_row=None)), 1, B) == -1 and "best_row must not be NULL" in _err(lib, h)
        for ok in (1e-6, 0.5, 1.0):
            assert lib.sqair_set_estimate(h, C.byref(_est(iou_min=ok)), 1, B) == 0
        assert lib.sqair_set_estimate(h, C.byref(_est(log_w=None)), 2, B) == 0      # NULL log_w: zeros
        # with SMC on, log_w must be the resampler's accumulator
        assert lib.sqair_set_smc(h, C.byref(_smc(log_w=0x2000)), B) == 0
        for other in (0x2100, None):
            assert lib.sqair_set_estimate(h, C.byref(_est(log_w=other)), 1, B) == -1 and "smc->log_w" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est(log_w=0x2000)), 1, B) == 0
        assert lib.sqair_set_estimate(h, None, 0, 0) == 0       # NULL: off


def test_pass_time_refusals_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            for T in (1, 3):   # a pass whose T is not the registered one
                assert fn(*_fwd_args(h, B, T=T)) == -1
                assert "sqair_set_estimate" in _err(lib, h) and "T = 2" in _err(lib, h) and "T = {}".format(T) in _err(lib, h)
            # a pass of another B is the state's to refuse
            assert fn(*_fwd_args(h, B + 1, T=2)) == -1 and "B = 5" in _err(lib, h) and "sqair_set_estimate" not in _err(lib, h)
            assert fn(*_fwd_args(h, B, T=2, bind=("where",))) == -1
            assert "sqair_set_estimate" in _err(lib, h) and "log_weights_per_timestep" in _err(lib, h)
        assert lib.sqair_set_estimate(h, C.byref(_est(mean_canvas=0x4000)), 2, B) == 0
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            assert fn(*_fwd_args(h, B, T=2)) == -1 and "sqair_set_estimate" in _err(lib, h) and "out->canvas" in _err(lib, h)
        # SMC switched on after the estimate, on another accumulator: refused at pass time
        assert lib.sqair_set_estimate(h, C.byref(_est(log_w=0x2000)), 2, B) == 0
        assert lib.sqair_set_smc(h, C.byref(_smc(log_w=0x2100)), B) == 0
        assert lib.sqair_forward(*_fwd_args(h, B, T=2)) == -1 and "sqair_set_estimate" in _err(lib, h) and "smc->log_w" in _err(lib, h)


def test_the_state_going_off_or_to_another_b_takes_the_estimate_with_it():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        # a pass of the registered B, another T and a NULL parameter pointer: the estimate refuses it while it is on; once it is
        # off the pass gets to its own argument check, which comes next -- still on the host
        null_flat = lambda b: (h, None) + _fwd_args(h, b, T=3)[2:]
        est_refuses = lambda b: lib.sqair_forward(*null_flat(b)) == -1 and "sqair_set_estimate" in _err(lib, h)
        gone = lambda b: lib.sqair_forward(*null_flat(b)) == -1 and "null argument" in _err(lib, h)
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0
        assert est_refuses(B)
        _state(lib, h, B)                  # the same B again: the estimate stays
        assert est_refuses(B)
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
        assert gone(B)
        _state(lib, h, B)                  # the state off and on again: the estimate is gone
        assert gone(B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0
        assert est_refuses(B)
        _state(lib, h, B + 1)              # another B: off
        assert gone(B + 1)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == -1 and "B = 4" in _err(lib, h) and "B = 5" in _err(lib, h)


def test_training_calls_never_estimate():
    """A training pass with the handle's state on is the state's to refuse; a carried training call does not look at the handle's
    estimate at all (there is none without a state)."""
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_estimate(h, C.byref(_est()), 2, B) == 0
        assert lib.sqair_forward_train(*_fwd_args(h, B, T=2)) == -1 and "carried state" in _err(lib, h)


@pytest.mark.parametrize("path", LIBS)
def test_kernel_entry_point_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        good = dict(where=DUMMY, presence=DUMMY, obj_id=DUMMY, what=DUMMY, canvas=DUMMY, lw=DUMMY, T=1, B=3, K=5)
        order = ("where", "presence", "obj_id", "what", "canvas", "lw", "T", "B", "K")
        call = lambda est, **kw: lib.sqair_lane_estimate_test(h, *[dict(good, **kw)[k] for k in order],
                                                              C.byref(est) if est is not None else None, DUMMY)
        assert lib.sqair_lane_estimate_test(None, *[good[k] for k in order], C.byref(_est()), DUMMY) == -1
        for kw in (dict(where=None), dict(presence=None), dict(obj_id=None), dict(lw=None), dict(T=0), dict(B=0), dict(K=0), dict(K=257),
                   dict(B=1 << 30, K=256)):
            assert call(_est(), **kw) == -1 and "sqair_lane_estimate_test" in _err(lib, h), kw
        assert call(None) == -1
        for bad in (0.0, 1.5, float("nan")):
            assert call(_est(iou_min=bad)) == -1 and "iou_min" in _err(lib, h)
        assert call(_est(best_row=None)) == -1 and "best_row" in _err(lib, h)
        assert call(_est(what=0x4000), what=None) == -1 and "est->what needs what" in _err(lib, h)
        assert call(_est(mean_canvas=0x4000), canvas=None) == -1 and "est->mean_canvas needs canvas" in _err(lib, h)


def test_stream_argument_errors():
    """The estimate's arguments are checked before the stream touches its core."""
    class Core(object):
        class cfg(object):
            sample_from_prior = False
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"^SqairStream: estimate_iou must lie in \(0, 1\]"):
            SqairStream(Core(), 2, estimate=True, estimate_iou=bad)
    with pytest.raises(ValueError, match=r"^SqairStream: estimate_canvas is for a stream with estimate=True"):
        SqairStream(Core(), 2, estimate_canvas=True)
