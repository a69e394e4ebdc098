"""No GPU: the forecast's C-ABI (include/sqair_hip.h: sqair_forecast) -- exported and declared, sized, and every refusal made
before any HIP call."""
import ctypes as C
import functools

import pytest

from sqair_amd import _capi
from tests import abi_host
from tests.abi_host import constant, err as _err, fields as header_fields, functions

NEW = ("sqair_forecast_workspace_bytes", "sqair_forecast")
LIBS = {"product": (_capi.LIB_PATH, dict()), "wide": (_capi.WIDE_LIB_PATH, dict(n_what=64))}
handle = functools.partial(abi_host.handle, hw=(32, 40))


def test_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    for name in NEW:
        assert name in _capi.EXPORTED_SYMBOLS
        assert name in functions(), name
    fields = header_fields("SqairForecastOutputs")
    assert [n for _, n in fields] == [n for n, _ in _capi.SqairForecastOutputs._fields_]
    assert all(ty.endswith("*") for ty, _ in fields)      # pointers, every one
    assert _capi.ABI_VERSION == 2
    assert constant("SQAIR_ABI_VERSION") == 2
    assert _capi.lib().sqair_abi_version() == 2


@pytest.mark.parametrize("which", sorted(LIBS))
def test_workspace_bytes_positive_and_growing(which):
    path, flags = LIBS[which]
    with handle(path, k_particles=3, n_steps_per_image=2, **flags) as (lib, h):
        ws = lambda F, B: lib.sqair_forecast_workspace_bytes(h, F, B)
        assert ws(1, 1) > 0
        assert ws(2, 1) > ws(1, 1) and ws(10, 1) > ws(2, 1)
        assert ws(1, 2) > ws(1, 1) and ws(3, 4) > ws(3, 2)
        assert ws(0, 1) == -1 and ws(1, 0) == -1


def _call(lib, h, F=2, B=1, noise=1, ws=None, out=True, ws_bytes=None):
    o = _capi.SqairForecastOutputs()
    nb = lib.sqair_forecast_workspace_bytes(h, max(F, 1), max(B, 1)) if ws_bytes is None else ws_bytes
    # (fake device addresses: every call below is refused before anything is dereferenced or launched)
    return lib.sqair_forecast(h, C.c_void_p(16), C.c_void_p(16), C.c_void_p(noise) if noise else None, F, B, None,
                              C.byref(o) if out else None, C.c_void_p(16) if ws is None else ws, nb, None)


def test_refusals_before_any_hip_call():
    with handle(_capi.LIB_PATH, k_particles=2, n_steps_per_image=2) as (lib, h):
        # no state set at all
        assert _call(lib, h) == -1 and "state_in" in _err(lib, h)
        # a state without state_in (export only)
        nb = lib.sqair_state_bytes(h, 2)
        assert lib.sqair_set_state(h, None, C.c_void_p(64), None, nb, 2) == 0
        assert _call(lib, h, B=2) == -1 and "state_in" in _err(lib, h)
        assert lib.sqair_set_state(h, C.c_void_p(64), C.c_void_p(64), None, nb, 2) == 0
        # a B other than the state's
        assert _call(lib, h, B=3) == -1 and "B = 3" in _err(lib, h)
        # F < 1
        assert _call(lib, h, F=0, B=2) == -1 and "F must be" in _err(lib, h)
        assert _call(lib, h, F=-4, B=2) == -1 and "F must be" in _err(lib, h)
        # NULL noise
        assert _call(lib, h, B=2, noise=0) == -1 and "noise" in _err(lib, h)
        # a workspace one byte short
        need = lib.sqair_forecast_workspace_bytes(h, 2, 2)
        assert _call(lib, h, B=2, ws_bytes=need - 1) == -1 and "workspace_bytes" in _err(lib, h)
        # switching the state off refuses again
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
        assert _call(lib, h, B=2) == -1 and "state_in" in _err(lib, h)


def test_refused_with_sample_from_prior():
    with handle(_capi.LIB_PATH, k_particles=2, n_steps_per_image=2, sample_from_prior=True) as (lib, h):
        assert _call(lib, h) == -1 and "sample_from_prior" in _err(lib, h)
