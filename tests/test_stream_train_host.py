"""Training with a carried state (include/sqair_hip.h: SqairCarry, sqair_forward_train_carry / sqair_backward_carry), host side:
the symbols and every refusal.  All of them are decided before any HIP call, so dummy device pointers are enough and no GPU is
needed."""
import ctypes as C
import os
import re

import pytest

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config

NEW = ("sqair_forward_train_carry", "sqair_backward_carry")
DUMMY = C.c_void_p(0x1000)     # never dereferenced: the calls below are refused first
OTHER = C.c_void_p(0x2000)
BIG = 1 << 40
B = 4


def _handle(path=None, hw=(50, 50), **flags):
    lib = _capi.lib(path)
    cfg = make_config(make_flags(**flags), hw)
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


def _err(lib, h):
    return lib.sqair_last_error(h).decode()


def _smc(**kw):
    f = dict(ess_frac=1.0, seed=0, uniforms=None, log_w=DUMMY.value, log_z=DUMMY.value, log_evidence=DUMMY.value,
             ess=DUMMY.value, u_out=None, resampled=DUMMY.value, src_rows=DUMMY.value)
    f.update(kw)
    return _capi.SqairSmc(**f)


def _carry(lib, h, smc=None, **kw):
    f = dict(state_in=DUMMY.value, state_out=DUMMY.value, src_rows=DUMMY.value, state_bytes=lib.sqair_state_bytes(h, B), B=B)
    f.update(kw)
    c = _capi.SqairCarry(**f)
    if smc is not None:
        c.smc = C.pointer(smc)
    return c


def _calls(lib, h, carry, lw=True, b=B):
    """(forward, backward) return codes for one carry; the forward's outputs bind log_weights_per_timestep when `lw`."""
    out = _capi.SqairOutputs(log_weights_per_timestep=DUMMY.value if lw else None)
    cp = C.byref(carry) if carry is not None else None
    f = lib.sqair_forward_train_carry(h, DUMMY, DUMMY, DUMMY, DUMMY, 2, b, cp, C.byref(out), DUMMY, BIG, DUMMY)
    fe = _err(lib, h)
    g = lib.sqair_backward_carry(h, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 2, b, cp, DUMMY, BIG, DUMMY, BIG, DUMMY, DUMMY)
    return f, fe, g, _err(lib, h)


def test_carry_symbols_are_exported_and_declared(repo_root):
    txt = open(os.path.join(repo_root, "include", "sqair_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\}\s*SqairCarry\s*;", txt)
    for path in (None, _capi.WIDE_LIB_PATH):
        lib = _capi.lib(path)
        for n in NEW:
            assert re.search(r"\b" + n + r"\s*\(", txt), n
            assert n in _capi.EXPORTED_SYMBOLS
            assert hasattr(lib, n)
        assert lib.sqair_abi_version() == 2


def test_carry_struct_layout():
    """The ctypes mirror of SqairCarry: three pointers, the byte count, B, the SMC pointer (natural alignment, 48 bytes)."""
    names = [n for n, _ in _capi.SqairCarry._fields_]
    assert names == ["state_in", "state_out", "src_rows", "state_bytes", "B", "smc"]
    assert _capi.SqairCarry.state_bytes.offset == 24 and _capi.SqairCarry.B.offset == 32 and _capi.SqairCarry.smc.offset == 40
    assert C.sizeof(_capi.SqairCarry) == 48


@pytest.mark.parametrize("path,flags", [
    (None, dict(k_particles=2, n_steps_per_image=3)),
    (_capi.WIDE_LIB_PATH, dict(k_particles=2, n_steps_per_image=3, n_what=64))])
def test_carry_refusals(path, flags):
    lib, h = _handle(path, **flags)
    try:
        def refused(carry, words, **kw):
            f, fe, g, ge = _calls(lib, h, carry, **kw)
            assert f == -1 and g == -1, (words, fe, ge)
            for w in words:
                assert w in fe and w in ge, (w, fe, ge)

        refused(None, ["NULL carry"])
        refused(_carry(lib, h), ["B = 5", "B = 4"], b=B + 1)
        refused(_carry(lib, h, state_bytes=lib.sqair_state_bytes(h, B) - 4), ["state_bytes"])
        refused(_carry(lib, h, state_in=None), ["state_in"])
        refused(_carry(lib, h, smc=_smc(ess_frac=0.5)), ["ess_frac"])
        refused(_carry(lib, h, smc=_smc(ess_frac=0.0)), ["ess_frac"])
        for k in ("log_w", "log_z", "log_evidence", "ess", "resampled", "src_rows"):
            refused(_carry(lib, h, smc=_smc(**{k: None})), ["NULL"])
        refused(_carry(lib, h, smc=_smc(src_rows=OTHER.value)), ["src_rows"])
        # the forward with SMC needs the log weights it resamples on (the backward has no outputs)
        f, fe, g, ge = _calls(lib, h, _carry(lib, h, smc=_smc()), lw=False)
        assert f == -1 and "log_weights_per_timestep" in fe
        # a handle that carries an inference state: the two registrations never mix
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        refused(_carry(lib, h), ["sqair_set_state"])
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
        # sqair_set_state keeps refusing the plain training calls (tests/test_stream_host.py pins that too)
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        out = _capi.SqairOutputs()
        assert lib.sqair_forward_train(h, DUMMY, DUMMY, DUMMY, DUMMY, 2, B, 0, C.byref(out), DUMMY, BIG, DUMMY) == -1
        assert "training" in _err(lib, h)
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
    finally:
        lib.sqair_destroy(h)


def test_carry_refused_with_sample_from_prior():
    lib, h = _handle(k_particles=2, n_steps_per_image=3, sample_from_prior=True, generate_after=2)
    try:
        f, fe, g, ge = _calls(lib, h, _carry(lib, h))
        assert f == -1 and g == -1 and "sample_from_prior" in fe and "sample_from_prior" in ge
    finally:
        lib.sqair_destroy(h)


def test_carry_refused_for_frames_too_large_to_train():
    lib, h = _handle(hw=(256, 256), k_particles=2, n_steps_per_image=3)
    try:
        f, fe, g, ge = _calls(lib, h, _carry(lib, h))
        assert f == -1 and g == -1 and "training is limited" in fe and "training is limited" in ge
    finally:
        lib.sqair_destroy(h)
