"""No GPU: the track history's C-ABI (include/sqair_hip.h: sqair_history_bytes / sqair_set_history / sqair_history_trace) --
exported and declared, sized in int64, and every refusal made before any HIP call (dummy device pointers are enough) -- and the
argument errors of SqairStream(history=...)."""
import ctypes as C
import functools
import types

import pytest

from sqair_amd import _capi
from sqair_amd.carried import CarriedState
from sqair_amd.stream import SqairStream
from tests.abi_host import (BIG, DUMMY, constant, err as _err, estimate, fields as header_fields, functions, fwd_args, handle, paragraph,
                            set_state as _state)

NEW = ("sqair_history_bytes", "sqair_set_history", "sqair_history_trace")
OTHER = C.c_void_p(0x2000)
ALL, MAND = 31, 7


def test_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    lib = _capi.lib()
    for name in NEW:
        assert name in _capi.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert name in functions(), name
    assert [n for _, n in header_fields("SqairTraceOutputs")] == [n for n, _ in _capi.SqairTraceOutputs._fields_]
    for name, bit in _capi.HISTORY_FIELDS.items():
        macro = {"log_weights_per_timestep": "LOG_W"}.get(name, name.upper())
        assert constant("SQAIR_HIST_" + macro) == bit, name
    assert constant("SQAIR_HIST_MANDATORY") == 7 and constant("SQAIR_HIST_ALL") == 31
    assert sum(_capi.HISTORY_FIELDS[n] for n in _capi.HISTORY_MANDATORY) == MAND
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION") and lib.sqair_abi_version() == 2
    # the history stays out of training on streams, and the header says so
    assert "out of scope" in paragraph("track history", "SQAIR_HIST_WHERE")


@pytest.mark.parametrize("which", ["product", "wide"])
def test_history_bytes(which):
    path, flags = {"product": (None, dict()), "wide": (_capi.WIDE_LIB_PATH, dict(n_what=64))}[which]
    with handle(path, k_particles=5, n_steps_per_image=4, **flags) as (lib, h):
        nb = lambda L, T, B, f=ALL: lib.sqair_history_bytes(h, L, T, B, f)
        nw, N, K = int(flags.get("n_what", 50)), 4, 5
        # a slot holds at least the chosen fields in their own widths plus the map and the counters
        per_slot = lambda T, B, what=True, lw=True: 4 * B * K * (2 + T * (N * (4 + 1 + 1 + (nw if what else 0)) + (1 if lw else 0)))
        for L, T, B in ((1, 1, 1), (64, 1, 32), (7, 5, 3)):
            assert nb(L, T, B) >= L * per_slot(T, B)
            assert nb(L, T, B) < L * per_slot(T, B) * 1.02 + 4 * L * B * K + 4096      # ... and little more (the trace scratch, padding)
            assert nb(L, T, B, MAND) >= L * per_slot(T, B, False, False) and nb(L, T, B, MAND) <= nb(L, T, B, MAND | 16) < nb(L, T, B)
        assert nb(2, 1, 4) > nb(1, 1, 4) and nb(2, 2, 4) > nb(2, 1, 4) and nb(2, 2, 5) > nb(2, 2, 4)
        # int64: a ring far beyond 2^31 bytes is sized, not wrapped
        big = nb(1 << 20, 1, 32)
        assert big > (1 << 20) * per_slot(1, 32) > 1 << 37 and big % 4 == 0
        assert nb(1 << 24, 10, 32) > 1 << 44
        # bad arguments
        assert nb(0, 1, 1) == -1 and nb(1, 0, 1) == -1 and nb(1, 1, 0) == -1 and nb(-3, 1, 1) == -1
        assert nb(1, 1, 1, 3) == -1 and nb(1, 1, 1, MAND | 32) == -1 and nb(1, 1, 1, 0) == -1
        assert lib.sqair_history_bytes(None, 1, 1, 1, ALL) == -1


def test_set_history_refusals_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        need = lib.sqair_history_bytes(h, 8, 1, B, ALL)
        # no state set
        assert lib.sqair_set_history(h, DUMMY, need, 8, ALL) == -1 and "carried state" in _err(lib, h)
        _state(lib, h, B)
        # L < 1
        for L in (0, -2):
            assert lib.sqair_set_history(h, DUMMY, BIG, L, ALL) == -1 and "L must be >= 1" in _err(lib, h)
        # ring_bytes too small (one word short of the smallest ring this L could be: one-frame passes)
        assert lib.sqair_set_history(h, DUMMY, need - 4, 8, ALL) == -1 and "ring_bytes" in _err(lib, h) and str(need) in _err(lib, h)
        # fields without the mandatory three, or with a bit nobody defined
        for f in (0, 3, 5, 6, 8 | 16, MAND | 32):
            assert lib.sqair_set_history(h, DUMMY, BIG, 8, f) == -1 and "fields" in _err(lib, h)
        assert lib.sqair_set_history(h, DUMMY, need, 8, ALL) == 0
        assert lib.sqair_set_history(h, DUMMY, need, 8, MAND) == 0
        assert lib.sqair_set_history(h, None, 0, 0, 0) == 0      # NULL ring: off


_fwd_args = functools.partial(fwd_args, bind=())      # nothing bound but what a call names


def test_pass_time_refusals_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        need1 = lib.sqair_history_bytes(h, 8, 1, B, ALL)
        assert lib.sqair_set_history(h, DUMMY, need1, 8, ALL) == 0
        every = ("where", "presence", "obj_id", "what", "log_weights_per_timestep")
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            # a B other than the state's
            assert fn(*_fwd_args(h, B + 1, bind=every)) == -1 and "B = 5" in _err(lib, h)
            # an output among the fields not bound
            for missing in every:
                assert fn(*_fwd_args(h, B, bind=[n for n in every if n != missing])) == -1
                assert "history" in _err(lib, h) and "must bind" in _err(lib, h), missing
            # a ring sized for one-frame passes cannot take three-frame ones
            assert fn(*_fwd_args(h, B, T=3, bind=every)) == -1 and "ring_bytes" in _err(lib, h)
        # with the mandatory fields only, what and the log weights may stay unbound: the refusal then is not the history's
        assert lib.sqair_set_history(h, DUMMY, BIG, 8, MAND) == 0
        assert lib.sqair_forward(*_fwd_args(h, B, bind=("where", "presence"))) == -1 and "must bind" in _err(lib, h)
        # the state going off takes the history with it: the trace is refused again
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
        o = _capi.SqairTraceOutputs(T=1)
        assert lib.sqair_history_trace(h, DUMMY, None, 1, C.byref(o), None) == -1 and "no history" in _err(lib, h)
        # ... and so does a state for another B
        _state(lib, h, B)
        assert lib.sqair_set_history(h, DUMMY, BIG, 8, ALL) == 0
        _state(lib, h, B + 1)
        assert lib.sqair_history_trace(h, DUMMY, None, 1, C.byref(o), None) == -1 and "no history" in _err(lib, h)


def test_a_refused_pass_leaves_the_handle_unchanged():
    """A pass the history would take and the estimate refuses must not fix the ring's frames per pass: the next pass, of the
    estimate's T, gets past every refusal to the pass's own argument check."""
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_history(h, DUMMY, BIG, 8, ALL) == 0
        assert lib.sqair_set_estimate(h, C.byref(estimate()), 1, B) == 0
        every = [n for n, _ in _capi.SqairOutputs._fields_]
        assert lib.sqair_forward(*_fwd_args(h, B, T=3, bind=every)) == -1
        assert "sqair_set_estimate" in _err(lib, h) and "registered for passes of T = 1" in _err(lib, h)
        args = _fwd_args(h, B, T=1, bind=every)
        assert lib.sqair_forward(*(args[:9] + (None,) + args[10:])) == -1      # (a NULL workspace)
        assert _err(lib, h) == "sqair_forward: null argument or bad T/B", _err(lib, h)
        assert "ring" not in _err(lib, h)


def test_training_passes_stay_refused_with_a_history_set():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_history(h, DUMMY, BIG, 8, ALL) == 0
        assert lib.sqair_forward_train(*_fwd_args(h, B)) == -1 and "training" in _err(lib, h)


def test_trace_refusals_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B, L = 4, 8
        o = _capi.SqairTraceOutputs(T=1, max_tracks=4)
        call = lambda ring=DUMMY, lag=1, out=o: lib.sqair_history_trace(h, ring, None, lag, C.byref(out) if out is not None else None, None)
        assert call() == -1 and "no history" in _err(lib, h)
        _state(lib, h, B)
        assert call() == -1 and "no history" in _err(lib, h)
        assert lib.sqair_set_history(h, DUMMY, lib.sqair_history_bytes(h, L, 1, B, MAND), L, MAND) == 0
        assert call(ring=OTHER) == -1 and "ring" in _err(lib, h)
        assert call(ring=None) == -1 and "ring" in _err(lib, h)
        for lag in (0, -1, L + 1):
            assert call(lag=lag) == -1 and "lag" in _err(lib, h)
        assert call(out=None) == -1 and "out" in _err(lib, h)
        assert call(out=_capi.SqairTraceOutputs(T=0)) == -1 and "out->T" in _err(lib, h)
        assert call(out=_capi.SqairTraceOutputs(T=2)) == -1 and "too small" in _err(lib, h)      # the ring holds one-frame passes
        # what / log_w of a ring set without them
        assert call(out=_capi.SqairTraceOutputs(T=1, what=0x1000)) == -1 and "without the field" in _err(lib, h)
        assert call(out=_capi.SqairTraceOutputs(T=1, log_w=0x1000)) == -1 and "without the field" in _err(lib, h)
        # the track table wants 1 <= max_tracks <= 1024
        for m in (0, -1, 1025):
            assert call(out=_capi.SqairTraceOutputs(T=1, max_tracks=m, track_id=0x1000)) == -1 and "max_tracks" in _err(lib, h)


def test_stream_argument_errors():
    """SqairStream checks history / history_fields before it touches its core."""
    core = types.SimpleNamespace(cfg=types.SimpleNamespace(sample_from_prior=False), K=2)
    for bad in (0, -1, 2.5, True, "8"):
        with pytest.raises(ValueError, match=r"^SqairStream: history must be an integer >= 1"):
            SqairStream(core, 2, history=bad)
    with pytest.raises(ValueError, match=r"^SqairStream: unknown history_fields \['canvas'\]"):
        SqairStream(core, 2, history=4, history_fields=("where", "canvas"))
    # the mandatory three are always kept, in the ring's order
    assert CarriedState.check_history(3, (), "X") == ("where", "presence", "obj_id")
    assert CarriedState.check_history(3, "what", "X") == ("where", "presence", "obj_id", "what")
    assert CarriedState.check_history(3, tuple(_capi.HISTORY_FIELDS), "X") == tuple(_capi.HISTORY_FIELDS)
