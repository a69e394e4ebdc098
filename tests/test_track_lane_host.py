"""No GPU: the C-ABI of the lane tracks (include/sqair_hip.h: sqair_history_trace_lane, sqair_track_lane_test) -- exported and
declared, sized, every refusal made before any HIP call -- and the Python side: the shapes helper and SqairStream.tracks' argument
errors."""
import ctypes as C
import functools
import types

import pytest

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from sqair_amd.stream import SqairStream
from tests import abi_host
from tests.abi_host import constant, err as _err, fields as header_fields, functions

NEW = ("sqair_trace_lane_scratch_bytes", "sqair_history_trace_lane", "sqair_track_lane_test")
LIBS = {"product": (_capi.LIB_PATH, dict()), "wide": (_capi.WIDE_LIB_PATH, dict(n_what=64))}
P = C.c_void_p(16)   # (a fake device address: every call below is refused before anything is dereferenced or launched)
B, K, N, L = 2, 3, 2, 4
handle = functools.partial(abi_host.handle, hw=(32, 40))


def test_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    for name in NEW:
        assert name in _capi.EXPORTED_SYMBOLS
        assert name in functions(), name
    assert [n for _, n in header_fields("SqairTraceLane")] == [n for n, _ in _capi.SqairTraceLane._fields_]
    assert _capi.SqairTraceLane._fields_[0] == ("iou_min", C.c_float)
    assert tuple(n for n, _ in _capi.SqairTraceLane._fields_[1:]) == _capi.TRACK_LANE_FIELDS
    # old callers pass the old struct: SqairTraceOutputs keeps its layout, the ABI its version
    assert [n for _, n in header_fields("SqairTraceOutputs")] == ["T", "max_tracks"] + list(_capi.TRACE_FIELDS)
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION") and _capi.lib().sqair_abi_version() == 2
    # the estimate's "out of scope" sentence points to the new call
    hdr = abi_host.raw()
    assert "sqair_history_trace_lane" in hdr[hdr.index("Out of scope: estimates for training passes"):][:300]


def test_track_lane_shapes():
    F, Bq, Kq, Nq = 6, 3, 5, 4
    s = _capi.track_lane_shapes(F, Bq, Kq, Nq)
    assert tuple(s) == _capi.TRACK_LANE_FIELDS and set(_capi.TRACK_LANE_INT_FIELDS) == {"best_row", "first_frame"}
    assert s == dict(best_row=(Bq,), weights=(Bq, Kq), obj_id=(Bq, Nq), presence=(Bq, Nq), box0=(Bq, Nq, 4), support=(Bq, Nq),
                     first_frame=(Bq, Nq), alive=(F, Bq, Nq), box_mean=(F, Bq, Nq, 4), box_std=(F, Bq, Nq, 4),
                     count_prob=(F, Bq, Nq + 1), valid_mass=(F, Bq))
    # the fields the two lane answers share have the forecast's shapes: past and future concatenate along the frame axis
    fc = _capi.forecast_lane_shapes(F, Bq, Kq, Nq)
    for n in ("best_row", "weights", "obj_id", "presence", "box0", "support", "alive", "box_mean", "box_std", "count_prob"):
        assert s[n] == fc[n], n


@pytest.mark.parametrize("which", sorted(LIBS))
def test_scratch_bytes(which):
    path, flags = LIBS[which]
    with handle(path, k_particles=3, n_steps_per_image=2, **flags) as (lib, h):
        nb = lib.sqair_trace_lane_scratch_bytes
        assert nb(h, 2, 5) > 0 and nb(h, 2, 5) % 4 == 0 and nb(h, 40, 5) > nb(h, 2, 5) and nb(h, 2, 256) > nb(h, 2, 5)
        assert nb(h, 2, 5) >= 4 * (2 * 5 + 2 * 2 * 5 * 2 + 2 * 2)          # the weights, the association, the ids, the objects
        assert nb(h, 0, 5) == -1 and nb(h, 2, 0) == -1 and nb(h, 2, 257) == -1


def _with_history(lib, h):
    """A handle with a (fake) state and ring registered: host-side bookkeeping only."""
    nb = lib.sqair_state_bytes(h, B)
    assert lib.sqair_set_state(h, C.c_void_p(64), C.c_void_p(64), None, nb, B) == 0
    bits = 7
    ring_bytes = lib.sqair_history_bytes(h, L, 2, B, bits)
    assert lib.sqair_set_history(h, C.c_void_p(128), ring_bytes, L, bits) == 0
    return C.c_void_p(128)


def _outs(T=1, **kw):
    o = _capi.SqairTraceOutputs(T=T, max_tracks=4)
    for n in ("where", "presence", "obj_id", "valid"):
        setattr(o, n, kw.get(n, 16))
    for n, v in kw.items():
        setattr(o, n, v)
    return o


def test_trace_lane_refusals_before_any_hip_call():
    with handle(_capi.LIB_PATH, k_particles=K, n_steps_per_image=N) as (lib, h):
        need = lib.sqair_trace_lane_scratch_bytes(h, B, K)
        good = _capi.SqairTraceLane(iou_min=0.5, best_row=32)

        def call(ring=None, lag=2, out=True, lane=good, scratch=P, nb=need, outs=None):
            o = _outs() if outs is None else outs
            return lib.sqair_history_trace_lane(h, ring, None, lag, C.byref(o) if out else None, None,
                                                None if lane is None else C.byref(lane), scratch, nb, None)

        # ---- everything sqair_history_trace refuses, under the new call's name
        assert call(ring=P) == -1 and "no history set" in _err(lib, h) and "sqair_history_trace_lane" in _err(lib, h)
        ring = _with_history(lib, h)
        assert call(ring=C.c_void_p(256)) == -1 and "ring must be the ring" in _err(lib, h)
        assert call(ring=None) == -1 and "ring must be the ring" in _err(lib, h)
        for lag in (0, -1, L + 1):
            assert call(ring=ring, lag=lag) == -1 and "lag = " in _err(lib, h)
        assert call(ring=ring, out=False) == -1 and "out must not be NULL" in _err(lib, h)
        assert call(ring=ring, outs=_outs(T=0)) == -1 and "out->T" in _err(lib, h)
        assert call(ring=ring, outs=_outs(T=3)) == -1 and "too small" in _err(lib, h)                 # the ring was sized for T = 2
        assert call(ring=ring, outs=_outs(what=16)) == -1 and "without the field" in _err(lib, h)
        assert call(ring=ring, outs=_outs(log_w=16)) == -1 and "without the field" in _err(lib, h)
        o = _outs(track_id=16)
        o.max_tracks = 0
        assert call(ring=ring, outs=o) == -1 and "max_tracks" in _err(lib, h)
        # ---- the lane's own
        assert call(ring=ring, lane=None) == -1 and "lane must not be NULL" in _err(lib, h)
        for bad in (0.0, -0.5, 1.5, float("nan")):
            assert call(ring=ring, lane=_capi.SqairTraceLane(iou_min=bad, best_row=32)) == -1 and "iou_min" in _err(lib, h)
        assert call(ring=ring, lane=_capi.SqairTraceLane(iou_min=0.5)) == -1 and "best_row" in _err(lib, h)
        assert call(ring=ring, nb=need - 1) == -1 and "scratch_bytes" in _err(lib, h) and "sqair_trace_lane_scratch_bytes" in _err(lib, h)
        assert call(ring=ring, scratch=None) == -1 and "scratch" in _err(lib, h)
        for name in ("where", "presence", "obj_id", "valid"):
            assert call(ring=ring, outs=_outs(**{name: None})) == -1 and "gathered rows" in _err(lib, h), name
        # the plain trace takes the same outputs with those pointers NULL: only the lane kernels need them (it would launch: not called)
        # ---- switching the history off refuses again
        assert lib.sqair_set_history(h, None, 0, 0, 0) == 0
        assert call(ring=ring) == -1 and "no history set" in _err(lib, h)


def test_more_than_256_particles_are_refused():
    """K > 256 never reaches the lane kernels: no handle is made for it (so no ring call can carry it), the kernel-level entry and the
    size query refuse it."""
    lib = _capi.lib()
    cfg = make_config(make_flags(k_particles=257, n_steps_per_image=N), (32, 40))
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == -1
    with handle(_capi.LIB_PATH, k_particles=256, n_steps_per_image=N) as (lib, h):
        assert lib.sqair_trace_lane_scratch_bytes(h, B, 256) > 0 and lib.sqair_trace_lane_scratch_bytes(h, B, 257) == -1
        lane = _capi.SqairTraceLane(iou_min=0.5, best_row=32)
        assert lib.sqair_track_lane_test(h, P, P, P, P, None, 1, B, 257, C.byref(lane), P, 1 << 40, None) == -1
        assert "bad F / B / K" in _err(lib, h)


def test_kernel_test_entry_refusals():
    with handle(_capi.LIB_PATH, k_particles=2, n_steps_per_image=N) as (lib, h):
        lane = _capi.SqairTraceLane(iou_min=0.5, best_row=32)

        def call(ptrs=(P,) * 4, F=1, Bq=1, Kq=2, lane=lane, scratch=P, nb=None):
            nb = lib.sqair_trace_lane_scratch_bytes(h, max(Bq, 1), min(max(Kq, 1), 256)) if nb is None else nb
            return lib.sqair_track_lane_test(h, *ptrs, None, F, Bq, Kq, None if lane is None else C.byref(lane), scratch, nb, None)

        for i in range(4):
            assert call(ptrs=tuple(None if j == i else P for j in range(4))) == -1 and "null" in _err(lib, h)
        assert call(lane=None) == -1 and call(scratch=None) == -1
        for kw in (dict(F=0), dict(Bq=0), dict(Kq=0), dict(Kq=257), dict(F=65536), dict(F=65535, Bq=2 ** 15, Kq=256)):
            assert call(**kw) == -1 and "bad F / B / K" in _err(lib, h), kw
        assert call(lane=_capi.SqairTraceLane(iou_min=0.0, best_row=32)) == -1 and "iou_min" in _err(lib, h)
        assert call(lane=_capi.SqairTraceLane(iou_min=0.5)) == -1 and "best_row" in _err(lib, h)
        assert call(nb=lib.sqair_trace_lane_scratch_bytes(h, 1, 2) - 1) == -1 and "scratch_bytes" in _err(lib, h)


def test_stream_argument_errors():
    """SqairStream.tracks checks lane / lane_iou / start before it touches its core or the device."""
    st = SqairStream.__new__(SqairStream)
    st.core = types.SimpleNamespace(N=3)
    st.carried = types.SimpleNamespace(ring=object(), history=4)
    with pytest.raises(ValueError, match=r"^SqairStream\.tracks: lane=True requires start='next'"):
        st.tracks(lane=True, start="last")
    for bad in (0.0, -1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"^SqairStream\.tracks: lane_iou must lie in \(0, 1\]"):
            st.tracks(lane=True, lane_iou=bad)
    with pytest.raises(ValueError, match=r"^SqairStream\.tracks: start must be"):
        st.tracks(lane=True, start="first")
