"""SMC resampling of a carried state (include/sqair_hip.h: sqair_set_smc), host side: the symbol, the struct layout, and every
refusal -- all of them are decided before any HIP call, so dummy device pointers are enough and no GPU is needed."""
import ctypes as C
import os
import re

import pytest

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config

DUMMY = C.c_void_p(0x1000)     # never dereferenced: the calls below are refused first
SRC = C.c_void_p(0x2000)       # the state's source map
BIG = 1 << 40
LIBS = [None, _capi.WIDE_LIB_PATH]
FLAGS = {None: dict(k_particles=3, n_steps_per_image=3), _capi.WIDE_LIB_PATH: dict(k_particles=3, n_steps_per_image=3, n_what=64)}
C_TYPES = {"float": (4, 4), "uint64_t": (8, 8), "int32_t*": (8, 8), "float*": (8, 8)}   # (size, alignment) on the 64-bit ABIs


def _handle(path=None, **flags):
    lib = _capi.lib(path)
    cfg = make_config(make_flags(**flags), (50, 50))
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


def _err(lib, h):
    return lib.sqair_last_error(h).decode()


def _smc(**kw):
    f = dict(ess_frac=0.5, seed=7, uniforms=None, log_w=0x3000, log_z=0x3100, log_evidence=0x3200, ess=0x3300, u_out=None,
             resampled=0x3400, src_rows=SRC.value)
    f.update(kw)
    return _capi.SqairSmc(**f)


def _set_state(lib, h, B, state_in=DUMMY, src=SRC):
    return lib.sqair_set_state(h, state_in, DUMMY, src, lib.sqair_state_bytes(h, B), B)


def _fwd_args(h, B, out, obs=DUMMY):
    return (h, DUMMY, DUMMY, obs, DUMMY, 1, B, 0, C.byref(out), DUMMY, BIG, DUMMY)


def test_smc_symbol_is_exported_and_declared(repo_root):
    txt = open(os.path.join(repo_root, "include", "sqair_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bsqair_set_smc\s*\(", txt)
    assert "sqair_set_smc" in _capi.EXPORTED_SYMBOLS
    for path in LIBS:
        assert hasattr(_capi.lib(path), "sqair_set_smc")
    assert _capi.lib().sqair_abi_version() == 2


def test_ctypes_struct_matches_the_header(repo_root):
    """Field names, order, sizes and offsets of SqairSmc as the header declares it (C layout rules on the 64-bit ABIs)."""
    txt = open(os.path.join(repo_root, "include", "sqair_hip.h")).read()
    body = re.search(r"typedef struct \{(.*?)\} SqairSmc;", txt, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)", decl)
        assert m, decl
        fields.append((m.group(3), m.group(1) + m.group(2)))
    off, align_max, want = 0, 1, []
    for name, ty in fields:
        size, align = C_TYPES[ty]
        off = (off + align - 1) // align * align
        want.append((name, off))
        off += size
        align_max = max(align_max, align)
    size = (off + align_max - 1) // align_max * align_max
    got = [(n, getattr(_capi.SqairSmc, n).offset) for n, _ in _capi.SqairSmc._fields_]
    assert got == want
    assert C.sizeof(_capi.SqairSmc) == size == 80


@pytest.mark.parametrize("path", LIBS, ids=["product", "wide"])
def test_set_smc_refusals(path):
    lib, h = _handle(path, **FLAGS[path])
    B = 4
    try:
        smc = _smc()
        # no state
        assert lib.sqair_set_smc(h, C.byref(smc), B) == -1
        assert "sqair_set_state" in _err(lib, h)
        # a state without state_in (export only), or without a source map
        assert lib.sqair_set_state(h, None, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        assert lib.sqair_set_smc(h, C.byref(smc), B) == -1
        assert "state_in" in _err(lib, h)
        assert _set_state(lib, h, B, src=None) == 0
        assert lib.sqair_set_smc(h, C.byref(smc), B) == -1
        assert "source map" in _err(lib, h)
        assert _set_state(lib, h, B) == 0
        # src_rows other than the state's map
        assert lib.sqair_set_smc(h, C.byref(_smc(src_rows=0x2004)), B) == -1
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
    finally:
        lib.sqair_destroy(h)


@pytest.mark.parametrize("path", LIBS, ids=["product", "wide"])
def test_pass_with_smc_needs_the_log_weights(path):
    lib, h = _handle(path, **FLAGS[path])
    B = 4
    try:
        assert _set_state(lib, h, B) == 0
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        out = _capi.SqairOutputs()   # log_weights_per_timestep not bound
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            assert fn(*_fwd_args(h, B, out)) == -1
            assert "log_weights_per_timestep" in _err(lib, h)
        # the state's own refusals still come first
        assert lib.sqair_forward(*_fwd_args(h, B + 1, out)) == -1
        assert "B = 5" in _err(lib, h)
    finally:
        lib.sqair_destroy(h)


@pytest.mark.parametrize("path", LIBS, ids=["product", "wide"])
def test_switching_the_state_off_clears_smc(path):
    """With SMC on, a pass without log_weights_per_timestep is refused by SMC; once the state is switched off (or re-set against
    another source map) the same call gets past SMC -- and is refused for its null frames instead, still before any HIP call."""
    lib, h = _handle(path, **FLAGS[path])
    B = 4
    out = _capi.SqairOutputs()

    def smc_refuses():
        assert lib.sqair_forward(*_fwd_args(h, B, out, obs=None)) == -1
        return "log_weights_per_timestep" in _err(lib, h)

    try:
        assert _set_state(lib, h, B) == 0
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        assert smc_refuses()
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0   # state off: SMC off
        assert _set_state(lib, h, B) == 0
        assert not smc_refuses()
        assert "null argument" in _err(lib, h)
        # re-setting the same state keeps SMC; another source map, another B or no state_in drops it
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        assert _set_state(lib, h, B) == 0
        assert smc_refuses()
        assert _set_state(lib, h, B, src=C.c_void_p(0x2004)) == 0
        assert not smc_refuses()
        assert _set_state(lib, h, B) == 0
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        assert _set_state(lib, h, B - 1) == 0
        assert lib.sqair_forward(*_fwd_args(h, B - 1, out, obs=None)) == -1
        assert "null argument" in _err(lib, h)
        # the NULL smc switch
        assert _set_state(lib, h, B) == 0
        assert lib.sqair_set_smc(h, C.byref(_smc()), B) == 0
        assert lib.sqair_set_smc(h, None, 0) == 0
        assert not smc_refuses()
    finally:
        lib.sqair_destroy(h)
