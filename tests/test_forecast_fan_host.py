"""No GPU: the C-ABI of the object forecasts (include/sqair_hip.h: sqair_forecast_fan, sqair_forecast_lane_test) -- exported and
declared, sized, and every refusal made before any HIP call."""
import ctypes as C
import functools

import pytest

from sqair_amd import _capi
from tests import abi_host
from tests.abi_host import constant, err as _err, fields as header_fields, functions

NEW =("sqair_forecast_fan_workspace_bytes", "sqair_forecast_fan", "sqair_forecast_lane_scratch_bytes", "sqair_forecast_lane_test")
LIBS = {"product": (_capi.LIB_PATH, dict()), "wide": (_capi.WIDE_LIB_PATH, dict(n_what=64))}
P = C.c_void_p(16)   # (a fake device address: every call below is refused before anything is dereferenced or launched)
handle = functools.partial(abi_host.handle, hw=(32, 40))


def test_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    for name in NEW:
        assert name in _capi.EXPORTED_SYMBOLS
        assert name in functions(), name
    assert [n for _, n in header_fields("SqairForecastLane")] == [n for n, _ in _capi.SqairForecastLane._fields_]
    assert constant("SQAIR_FORECAST_FAN_MAX") == _capi.FORECAST_FAN_MAX == 1024
    # old callers pass the old struct: SqairForecastOutputs keeps its layout
    assert header_fields("SqairForecastOutputs") == [
        ("float*", "what"), ("float*", "where"), ("float*", "presence"), ("float*", "presence_prob"), ("float*", "presence_logit"),
        ("float*", "obj_id"), ("float*", "canvas"), ("float*", "glimpse"), ("const float*", "log_w"), ("float*", "mean_canvas"),
        ("float*", "expected_count")]
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION") and _capi.lib().sqair_abi_version() == 2


@pytest.mark.parametrize("which", sorted(LIBS))
def test_workspace_bytes(which):
    path, flags = LIBS[which]
    with handle(path, k_particles=3, n_steps_per_image=2, **flags) as (lib, h):
        fan, plain = lib.sqair_forecast_fan_workspace_bytes, lib.sqair_forecast_workspace_bytes
        for F, B in ((1, 1), (2, 3), (10, 2)):
            assert fan(h, F, B, 1) >= plain(h, F, B) > 0
            assert fan(h, F, B, 4) > fan(h, F, B, 2) > fan(h, F, B, 1)
            assert fan(h, F, B, 4) >= plain(h, F, B * 4)
        assert fan(h, 0, 1, 1) == -1 and fan(h, 1, 0, 1) == -1 and fan(h, 1, 1, 0) == -1 and fan(h, 1, 1, -2) == -1
        assert fan(h, 1, 1, 341) > 0 and fan(h, 1, 1, 342) == -1          # K * S <= 1024 with K = 3
        assert fan(h, 1, 2 ** 22, 341) == -1                              # R * S * N beyond int32
        assert lib.sqair_forecast_lane_scratch_bytes(h, 2, 5) > 0
        assert lib.sqair_forecast_lane_scratch_bytes(h, 0, 5) == -1 and lib.sqair_forecast_lane_scratch_bytes(h, 2, 257) == -1


def _call(lib, h, F=2, B=2, S=2, noise=True, out=True, ws=True, ws_bytes=None, lane=None, flat=True):
    o = _capi.SqairForecastOutputs()
    nb = lib.sqair_forecast_fan_workspace_bytes(h, max(F, 1), max(B, 1), min(max(S, 1), 300)) if ws_bytes is None else ws_bytes
    return lib.sqair_forecast_fan(h, P if flat else None, P, P if noise else None, F, B, S, None, C.byref(o) if out else None,
                                  None if lane is None else C.byref(lane), P if ws else None, nb, None)


def test_fan_refusals_before_any_hip_call():
    with handle(_capi.LIB_PATH, k_particles=2, n_steps_per_image=2) as (lib, h):
        # ---- everything sqair_forecast refuses
        assert _call(lib, h) == -1 and "state_in" in _err(lib, h) and "sqair_forecast_fan" in _err(lib, h)      # no state at all
        nb = lib.sqair_state_bytes(h, 2)
        assert lib.sqair_set_state(h, None, C.c_void_p(64), None, nb, 2) == 0                                    # export only
        assert _call(lib, h) == -1 and "state_in" in _err(lib, h)
        assert lib.sqair_set_state(h, C.c_void_p(64), C.c_void_p(64), None, nb, 2) == 0
        assert _call(lib, h, B=3) == -1 and "B = 3" in _err(lib, h)
        assert _call(lib, h, F=0) == -1 and "F must be" in _err(lib, h)
        assert _call(lib, h, F=-4) == -1 and "F must be" in _err(lib, h)
        assert _call(lib, h, noise=False) == -1 and "noise" in _err(lib, h)
        assert _call(lib, h, out=False) == -1 and "null" in _err(lib, h)
        assert _call(lib, h, ws=False) == -1 and "null" in _err(lib, h)
        assert _call(lib, h, flat=False) == -1 and "null" in _err(lib, h)
        # ---- the fan's own
        assert _call(lib, h, S=0) == -1 and "S must be" in _err(lib, h)
        assert _call(lib, h, S=-1) == -1 and "S must be" in _err(lib, h)
        assert _call(lib, h, S=513, ws_bytes=1 << 40) == -1 and "SQAIR_FORECAST_FAN_MAX" in _err(lib, h)         # K * S = 1026
        need = lib.sqair_forecast_fan_workspace_bytes(h, 2, 2, 2)
        assert _call(lib, h, ws_bytes=need - 1) == -1 and "workspace_bytes" in _err(lib, h) and "fan_workspace_bytes" in _err(lib, h)
        # a workspace that serves the plain forecast of the same rows is still too small for the fan
        assert _call(lib, h, S=1, ws_bytes=lib.sqair_forecast_workspace_bytes(h, 2, 2)) == -1 and "workspace_bytes" in _err(lib, h)
        # ---- with lane set
        best = C.c_void_p(32)
        for bad in (0.0, -0.5, 1.5, float("nan")):
            assert _call(lib, h, lane=_capi.SqairForecastLane(iou_min=bad, best_row=best)) == -1 and "iou_min" in _err(lib, h)
        assert _call(lib, h, lane=_capi.SqairForecastLane(iou_min=0.5)) == -1 and "best_row" in _err(lib, h)
        # switching the state off refuses again
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
        assert _call(lib, h) == -1 and "state_in" in _err(lib, h)


def test_fan_refuses_int32_overflow_and_sample_from_prior():
    with handle(_capi.LIB_PATH, k_particles=2, n_steps_per_image=2) as (lib, h):
        B = 2 ** 21
        nb = lib.sqair_state_bytes(h, B)
        assert lib.sqair_set_state(h, C.c_void_p(64), C.c_void_p(64), None, nb, B) == 0
        assert _call(lib, h, B=B, S=512, ws_bytes=1 << 62) == -1 and "int32" in _err(lib, h)                     # R * S * N = 2^32
    with handle(_capi.LIB_PATH, k_particles=2, n_steps_per_image=2, sample_from_prior=True) as (lib, h):
        assert _call(lib, h) == -1 and "sample_from_prior" in _err(lib, h)


def test_lane_test_entry_refusals():
    with handle(_capi.LIB_PATH, k_particles=2, n_steps_per_image=2) as (lib, h):
        lane = _capi.SqairForecastLane(iou_min=0.5, best_row=C.c_void_p(32))

        def call(ptrs=(P,) * 6, F=1, B=1, K=2, S=2, lane=lane, scratch=P, nb=None):
            nb = lib.sqair_forecast_lane_scratch_bytes(h, max(B, 1), min(max(K, 1), 256)) if nb is None else nb
            return lib.sqair_forecast_lane_test(h, *ptrs, None, F, B, K, S, None if lane is None else C.byref(lane), scratch, nb, None)

        for i in range(6):
            assert call(ptrs=tuple(None if j == i else P for j in range(6))) == -1 and "null" in _err(lib, h)
        assert call(lane=None) == -1 and call(scratch=None) == -1
        for kw in (dict(F=0), dict(B=0), dict(K=0), dict(K=257), dict(S=0), dict(K=256, S=5), dict(F=65536)):
            assert call(**kw) == -1 and "bad F / B / K / S" in _err(lib, h), kw
        assert call(lane=_capi.SqairForecastLane(iou_min=0.0, best_row=C.c_void_p(32))) == -1 and "iou_min" in _err(lib, h)
        assert call(lane=_capi.SqairForecastLane(iou_min=0.5)) == -1 and "best_row" in _err(lib, h)
        assert call(nb=lib.sqair_forecast_lane_scratch_bytes(h, 1, 2) - 1) == -1 and "scratch_bytes" in _err(lib, h)
