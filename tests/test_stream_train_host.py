"""Training with a carried state (include/sqair_hip.h: SqairCarry, sqair_forward_train_carry / sqair_backward_carry), host side:
the symbols and every refusal.  All of them are decided before any HIP call, so dummy device pointers are enough and no GPU is
needed."""
import ctypes as C

import pytest

from sqair_amd import _capi
from tests.abi_host import (BIG, CARRY_B as B, DUMMY, LIBS, OTHER, carry as _carry, err as _err, fields as header_fields, functions, fwd_args,
                            handle, train_smc)

NEW = ("sqair_forward_train_carry", "sqair_backward_carry")


def _calls(lib, h, carry, lw=True, b=B):
    """(forward, backward) return codes for one carry; the forward's outputs bind log_weights_per_timestep when `lw`."""
    out = _capi.SqairOutputs(log_weights_per_timestep=DUMMY.value if lw else None)
    cp = C.byref(carry) if carry is not None else None
    f = lib.sqair_forward_train_carry(h, DUMMY, DUMMY, DUMMY, DUMMY, 2, b, cp, C.byref(out), DUMMY, BIG, DUMMY)
    fe = _err(lib, h)
    g = lib.sqair_backward_carry(h, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 2, b, cp, DUMMY, BIG, DUMMY, BIG, DUMMY, DUMMY)
    return f, fe, g, _err(lib, h)


def test_carry_symbols_are_exported_and_declared():
    assert header_fields("SqairCarry")
    for path in LIBS:
        lib = _capi.lib(path)
        for n in NEW:
            assert n in functions(), n
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
    with handle(path, **flags) as (lib, h):
        def refused(carry, words, **kw):
            f, fe, g, ge = _calls(lib, h, carry, **kw)
            assert f == -1 and g == -1, (words, fe, ge)
            for w in words:
                assert w in fe and w in ge, (w, fe, ge)

        refused(None, ["NULL carry"])
        refused(_carry(lib, h), ["B = 5", "B = 4"], b=B + 1)
        refused(_carry(lib, h, state_bytes=lib.sqair_state_bytes(h, B) - 4), ["state_bytes"])
        refused(_carry(lib, h, state_in=None), ["state_in"])
        refused(_carry(lib, h, smc=train_smc(ess_frac=0.5)), ["ess_frac"])
        refused(_carry(lib, h, smc=train_smc(ess_frac=0.0)), ["ess_frac"])
        for k in ("log_w", "log_z", "log_evidence", "ess", "resampled", "src_rows"):
            refused(_carry(lib, h, smc=train_smc(**{k: None})), ["NULL"])
        refused(_carry(lib, h, smc=train_smc(src_rows=OTHER.value)), ["src_rows"])
        # the forward with SMC needs the log weights it resamples on (the backward has no outputs)
        f, fe, g, ge = _calls(lib, h, _carry(lib, h, smc=train_smc()), lw=False)
        assert f == -1 and "log_weights_per_timestep" in fe
        # a handle that carries an inference state: the two registrations never mix
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        refused(_carry(lib, h), ["sqair_set_state"])
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
        # sqair_set_state keeps refusing the plain training calls (tests/test_stream_host.py pins that too)
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        assert lib.sqair_forward_train(*fwd_args(h, B, T=2, bind=())) == -1
        assert "training" in _err(lib, h)
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0


def test_carry_refused_with_sample_from_prior():
    with handle(k_particles=2, n_steps_per_image=3, sample_from_prior=True, generate_after=2) as (lib, h):
        f, fe, g, ge = _calls(lib, h, _carry(lib, h))
        assert f == -1 and g == -1 and "sample_from_prior" in fe and "sample_from_prior" in ge


def test_carry_refused_for_frames_too_large_to_train():
    with handle(hw=(256, 256), k_particles=2, n_steps_per_image=3) as (lib, h):
        f, fe, g, ge = _calls(lib, h, _carry(lib, h))
        assert f == -1 and g == -1 and "training is limited" in fe and "training is limited" in ge
