"""No GPU: the C-ABI of training on gappy and ragged streams (include/sqair_hip.h: sqair_forward_train_carry_masked /
sqair_backward_carry_masked) -- exported and declared, the ABI version unchanged, every refusal made before any HIP call (dummy
device pointers are enough) -- and the argument errors of StreamTrainer(missing=...).step(observed=...)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from sqair_amd.train import StreamTrainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sqair_forward_train_carry_masked", "sqair_backward_carry_masked")
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


def _calls(lib, h, carry, lw=True, b=B, mask=DUMMY):
    """(forward, its error text, backward, its error text) of the masked pair for one carry."""
    out = _capi.SqairOutputs(log_weights_per_timestep=DUMMY.value if lw else None)
    cp = C.byref(carry) if carry is not None else None
    f = lib.sqair_forward_train_carry_masked(h, DUMMY, DUMMY, DUMMY, DUMMY, 2, b, cp, mask, C.byref(out), DUMMY, BIG, DUMMY)
    fe = _err(lib, h)
    g = lib.sqair_backward_carry_masked(h, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 2, b, cp, mask, DUMMY, BIG, DUMMY, BIG, DUMMY, DUMMY)
    return f, fe, g, _err(lib, h)


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    hdr = open(os.path.join(ROOT, "include", "sqair_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for path in (None, _capi.WIDE_LIB_PATH):
        lib = _capi.lib(path)
        for n in NEW:
            assert hasattr(lib, n) and n in _capi.EXPORTED_SYMBOLS
        assert lib.sqair_abi_version() == 2
    assert _capi.ABI_VERSION == 2 and re.search(r"#define SQAIR_ABI_VERSION 2\b", hdr)
    # the unmasked signatures with the mask after the carry
    assert re.search(r"\bint\s+sqair_forward_train_carry_masked\s*\([^)]*const SqairCarry\*\s*carry,\s*const int32_t\*\s*observed\s*,"
                     r"\s*const SqairOutputs\*\s*out,", code)
    assert re.search(r"\bint\s+sqair_backward_carry_masked\s*\([^)]*const SqairCarry\*\s*carry,\s*const int32_t\*\s*observed\s*,"
                     r"\s*void\*\s*train_workspace,", code)
    # SqairCarry itself did not change
    assert [n for n, _ in _capi.SqairCarry._fields_] == ["state_in", "state_out", "src_rows", "state_bytes", "B", "smc"]
    assert C.sizeof(_capi.SqairCarry) == 48
    # the one definition of the semantics sits above the calls
    doc = hdr[hdr.index("training on gappy and ragged streams: a per-frame"):hdr.index("int sqair_forward_train_carry_masked")]
    for word in ("DRAWN FROM p_theta", "LATER IN THE SAME", "log_weights_per_timestep = 0", "exactly zero", "s / T'", "NULL observed",
                 "T' + 1 kernel nodes"):
        assert word in doc, word
    # sqair_set_observed keeps refusing training calls, and its text points here
    doc = hdr[hdr.index("missing-frame steps"):hdr.index("int sqair_set_observed")]
    assert "out of scope" in doc and "sqair_forward_train_carry_masked" in doc


@pytest.mark.parametrize("path,flags", [
    (None, dict(k_particles=2, n_steps_per_image=3)),
    (_capi.WIDE_LIB_PATH, dict(k_particles=2, n_steps_per_image=3, n_what=64))])
@pytest.mark.parametrize("mask", [DUMMY, None])
def test_refusals_before_any_hip_call(path, flags, mask):
    """Everything the unmasked carried calls refuse, with a mask and with NULL for one, under the masked calls' names."""
    lib, h = _handle(path, **flags)
    try:
        def refused(carry, words, **kw):
            f, fe, g, ge = _calls(lib, h, carry, mask=mask, **kw)
            assert f == -1 and g == -1, (words, fe, ge)
            assert "sqair_forward_train_carry_masked" in fe and "sqair_backward_carry_masked" in ge
            for w in words:
                assert w in fe and w in ge, (w, fe, ge)

        refused(None, ["NULL carry"])
        refused(_carry(lib, h), ["B = 5", "B = 4"], b=B + 1)
        refused(_carry(lib, h, state_bytes=lib.sqair_state_bytes(h, B) - 4), ["state_bytes"])
        refused(_carry(lib, h, state_in=None), ["state_in"])
        refused(_carry(lib, h, smc=_smc(ess_frac=0.5)), ["ess_frac"])       # adaptive-ESS training stays out of scope
        refused(_carry(lib, h, smc=_smc(ess_frac=0.0)), ["ess_frac"])
        for k in ("log_w", "log_z", "log_evidence", "ess", "resampled", "src_rows"):
            refused(_carry(lib, h, smc=_smc(**{k: None})), ["NULL"])
        refused(_carry(lib, h, smc=_smc(src_rows=OTHER.value)), ["src_rows"])
        f, fe, g, ge = _calls(lib, h, _carry(lib, h, smc=_smc()), lw=False, mask=mask)
        assert f == -1 and "log_weights_per_timestep" in fe
        # a handle that carries an inference state, with or without its own mask: the registrations never mix
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        refused(_carry(lib, h), ["sqair_set_state"])
        assert lib.sqair_set_observed(h, DUMMY, 2, B) == 0
        f, fe, g, ge = _calls(lib, h, _carry(lib, h), mask=mask)
        assert f == -1 and g == -1 and "sqair_set_observed" in fe and "sqair_set_observed" in ge
        # ... and the handle's mask keeps refusing the unmasked training calls (tests/test_missing_host.py pins the text)
        out = _capi.SqairOutputs(log_weights_per_timestep=DUMMY.value)
        assert lib.sqair_forward_train(h, DUMMY, DUMMY, DUMMY, DUMMY, 2, B, 0, C.byref(out), DUMMY, BIG, DUMMY) == -1
        assert "out of scope" in _err(lib, h)
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
    finally:
        lib.sqair_destroy(h)


def test_refused_with_sample_from_prior_and_for_frames_too_large_to_train():
    lib, h = _handle(k_particles=2, n_steps_per_image=3, sample_from_prior=True, generate_after=2)
    try:
        f, fe, g, ge = _calls(lib, h, _carry(lib, h))
        assert f == -1 and g == -1 and "sample_from_prior" in fe and "sample_from_prior" in ge
    finally:
        lib.sqair_destroy(h)
    lib, h = _handle(hw=(256, 256), k_particles=2, n_steps_per_image=3)
    try:
        f, fe, g, ge = _calls(lib, h, _carry(lib, h))
        assert f == -1 and g == -1 and "training is limited" in fe and "training is limited" in ge
    finally:
        lib.sqair_destroy(h)


def test_trainer_argument_errors():
    """``observed`` is checked before the trainer touches its core, by the code SqairStream uses, under the trainer's name."""
    def trainer(missing, T=1, B=3):
        tr = StreamTrainer.__new__(StreamTrainer)
        tr.missing, tr.T, tr.B = missing, T, B
        return tr
    with pytest.raises(ValueError, match=r"^StreamTrainer.step: observed is for a trainer with missing=True"):
        trainer(False).step(None, observed=np.ones(3, bool))
    tr = trainer(True)
    assert tr._check_observed(None) is None
    assert tuple(tr._check_observed(np.array([True, False, True])).shape) == (1, 3)     # [B] when T' = 1
    assert torch.equal(tr._check_observed([[True, False, True]]), torch.tensor([[True, False, True]]))
    for bad in (np.ones(4, bool), np.ones((2, 3), bool), np.ones((1, 3, 1), bool)):
        with pytest.raises(ValueError, match=r"^StreamTrainer.step: observed of shape .* \[1, 3\] expected \(or \[3\]\)"):
            tr.step(None, observed=bad)
    for bad in (np.ones(3, np.int32), np.ones(3, np.float32)):
        with pytest.raises(ValueError, match=r"^StreamTrainer.step: observed must be a bool array"):
            tr.step(None, observed=bad)
    tr = trainer(True, T=4)
    assert tuple(tr._check_observed(np.ones((4, 3), bool)).shape) == (4, 3)
    with pytest.raises(ValueError, match=r"^StreamTrainer.step: observed of shape \(3,\) given, \[4, 3\] expected$"):
        tr.step(None, observed=np.ones(3, bool))   # [B] alone is for one-frame steps
    # one implementation: the stream's check is the same function
    from sqair_amd import carried, stream
    assert stream.check_observed is carried.check_observed
