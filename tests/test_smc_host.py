"""SMC resampling of a carried state (include/sqair_hip.h: sqair_set_smc), host side: the symbol, the struct layout, and every
refusal -- all of them are decided before any HIP call, so dummy device pointers are enough and no GPU is needed."""
import ctypes as C
import functools

import pytest

from sqair_amd import _capi
from tests.abi_host import (DUMMY, LIBS, c_layout, err as _err, fields as header_fields, functions, fwd_args, handle,
                            set_state as _set_state, smc as dummy_smc)

FLAGS = {None: dict(k_particles=3, n_steps_per_image=3), _capi.WIDE_LIB_PATH: dict(k_particles=3, n_steps_per_image=3, n_what=64)}


def _smc(**kw):
    """The harness's SqairSmc with the out buffers at addresses of their own."""
    return dummy_smc(**dict(dict(log_w=0x3000, log_z=0x3100, log_evidence=0x3200, ess=0x3300, resampled=0x3400), **kw))


_fwd_args = functools.partial(fwd_args, bind=())      # log_weights_per_timestep not bound


def test_smc_symbol_is_exported_and_declared():
    assert "sqair_set_smc" in functions()
    assert "sqair_set_smc" in _capi.EXPORTED_SYMBOLS
    for path in LIBS:
        assert hasattr(_capi.lib(path), "sqair_set_smc")
    assert _capi.lib().sqair_abi_version() == 2


def test_ctypes_struct_matches_the_header(tmp_path):
    """Field names, order, types, offsets and size of SqairSmc: the header's as the parser reads them and as the compiler lays them
    out, against the binding's."""
    fields = header_fields("SqairSmc")
    assert fields == [("float", "ess_frac"), ("uint64_t", "seed"), ("const float*", "uniforms"), ("float*", "log_w"), ("float*", "log_z"),
                      ("float*", "log_evidence"), ("float*", "ess"), ("float*", "u_out"), ("int32_t*", "resampled"), ("int32_t*", "src_rows")]
    names = [n for _, n in fields]
    assert names == [n for n, _ in _capi.SqairSmc._fields_]
    size, offsets = c_layout(tmp_path, dict(SqairSmc=names))["SqairSmc"]
    assert offsets == [getattr(_capi.SqairSmc, n).offset for n in names]
    assert C.sizeof(_capi.SqairSmc) == size == 80


@pytest.mark.parametrize("path", LIBS, ids=["product", "wide"])
def test_set_smc_refusals(path):
    B = 4
    with handle(path, **FLAGS[path]) as (lib, h):
        smc = _smc()
        # no state
        assert lib.sqair_set_smc(h, C.byref(smc), B) == -1
        assert "sqair_set_state" in _err(lib, h)
        # a state without state_in (export only), or without a source map
        _set_state(lib, h, B, state_in=None, src=None)
        assert lib.sqair_set_smc(h, C.byref(smc), B) == -1
        assert "state_in" in _err(lib, h)
        _set_state(lib, h, B, src=None)
        assert lib.sqair_set_smc(h, C.byref(smc), B) == -1
        assert "source map" in _err(lib, h)
        _set_state(lib, h, B)
        # src_rows other than the state's map
        assert lib.sqair_set_smc(h, C.byref(_smc(src_rows=DUMMY.value + 4)), B) == -1
        assert "src_rows" in _err(lib, h)
        # ess_frac NaN or outside [0, 1]
        for bad in (float("nan"), -0.01, 1.01, float("inf")):
            assert lib.sqair_set_smc(h, C.byref(_smc(ess_frac=bad)), B) == -1
            assert "ess_frac" in _err(lib, h)
        # a NULL out buffer
        for name in ("log_w", "log_z", "log_evidence", "ess", "resampled"):
            assert lib.sqair_set_smc(h, C.byref(_smc(**{name: None})), B) == -1
            assert name in _err(lib, h)
        # B other than the state's
        assert lib.sqair_set_smc(h, C.byref(smc), B + 1) == -1
        assert "B = 5" in _err(lib, h)
        # accepted: both ends of ess_frac, caller's uniforms or Philox, u_out optional; NULL = off
        for ok in (_smc(ess_frac=0.0), _smc(ess_frac=1.0, uniforms=0x3500, u_out=0x3600), smc):
            assert lib.sqair_set_smc(h, C.byref(ok), B) == 0, _err(lib, h)
        assert lib.sqair_set_smc(h, None, B) == 0


@pytest.mark.parametrize("path", LIBS, ids=["product", "wide"])
def test_pass_with_smc_needs_the_log_weights(path):
    B = 4
    with handle(path, **FLAGS[path]) as (lib, h):
        _set_state(lib, h, B)
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            assert fn(*_fwd_args(h, B)) == -1
            assert "log_weights_per_timestep" in _err(lib, h)
        # the state's own refusals still come first
        assert lib.sqair_forward(*_fwd_args(h, B + 1)) == -1
        assert "B = 5" in _err(lib, h)


@pytest.mark.parametrize("path", LIBS, ids=["product", "wide"])
def test_switching_the_state_off_clears_smc(path):
    """With SMC on, a pass without log_weights_per_timestep is refused by SMC; once the state is switched off (or re-set against
    another source map) the same call gets past SMC -- and is refused for its null frames instead, still before any HIP call."""
    B = 4
    with handle(path, **FLAGS[path]) as (lib, h):
        def smc_refuses():
            assert lib.sqair_forward(*_fwd_args(h, B, obs=None)) == -1
            return "log_weights_per_timestep" in _err(lib, h)

        _set_state(lib, h, B)
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        assert smc_refuses()
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0   # state off: SMC off
        _set_state(lib, h, B)
        assert not smc_refuses()
        assert "null argument" in _err(lib, h)
        # re-setting the same state keeps SMC; another source map, another B or no state_in drops it
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        _set_state(lib, h, B)
        assert smc_refuses()
        _set_state(lib, h, B, src=C.c_void_p(DUMMY.value + 4))
        assert not smc_refuses()
        _set_state(lib, h, B)
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        _set_state(lib, h, B - 1)
        assert lib.sqair_forward(*_fwd_args(h, B - 1, obs=None)) == -1
        assert "null argument" in _err(lib, h)
        # the NULL smc switch
        _set_state(lib, h, B)
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        assert lib.sqair_set_smc(h, None, 0) == 0
        assert not smc_refuses()
