"""No GPU: the C-ABI of training on gappy and ragged streams (include/sqair_hip.h: sqair_forward_train_carry_masked /
sqair_backward_carry_masked) -- exported and declared, the ABI version unchanged, every refusal made before any HIP call (dummy
device pointers are enough) -- and the argument errors of StreamTrainer(missing=...).step(observed=...)."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.train import StreamTrainer
from tests.abi_host import BIG, DUMMY, LIBS, constant, err as _err, fwd_args, handle, paragraph, phrases, prototype
from tests.abi_host import CARRY_B as B, OTHER, carry as _carry, train_smc      # the unmasked calls' carry and SMC: the masked ones take the same

NEW = ("sqair_forward_train_carry_masked", "sqair_backward_carry_masked")


def _calls(lib, h, carry, lw=True, b=B, mask=DUMMY):
    """(forward, its error text, backward, its error text) of the masked pair for one carry."""
    out = _capi.SqairOutputs(log_weights_per_timestep=DUMMY.value if lw else None)
    cp = C.byref(carry) if carry is not None else None
    f = lib.sqair_forward_train_carry_masked(h, DUMMY, DUMMY, DUMMY, DUMMY, 2, b, cp, mask, C.byref(out), DUMMY, BIG, DUMMY)
    fe = _err(lib, h)
    g = lib.sqair_backward_carry_masked(h, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 2, b, cp, mask, DUMMY, BIG, DUMMY, BIG, DUMMY, DUMMY)
    return f, fe, g, _err(lib, h)


def test_the_symbols_are_exported_and_declared_and_the_abi_is_unchanged():
    for path in LIBS:
        lib = _capi.lib(path)
        for n in NEW:
            assert hasattr(lib, n) and n in _capi.EXPORTED_SYMBOLS
        assert lib.sqair_abi_version() == 2
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    # the unmasked signatures with the mask after the carry
    assert prototype("sqair_forward_train_carry_masked") == (
        "int sqair_forward_train_carry_masked(SqairHandle* h, const float* flat_params, const void* packed, const float* obs, "
        "const float* noise, int T, int B, const SqairCarry* carry, const int32_t* observed, const SqairOutputs* out, "
        "void* train_workspace, int64_t workspace_bytes, void* stream)")
    assert prototype("sqair_backward_carry_masked") == (
        "int sqair_backward_carry_masked(SqairHandle* h, const float* flat_params, const void* packed, const float* obs, "
        "const float* noise, const float* importance_weights, const float* vimco_signal, int T, int B, const SqairCarry* carry, "
        "const int32_t* observed, void* train_workspace, int64_t workspace_bytes, void* scratch, int64_t scratch_bytes, "
        "float* flat_grad, void* stream)")
    for name in NEW:      # ... which is all that differs from the unmasked calls
        assert prototype(name).replace("_masked", "").replace(" const int32_t* observed,", "") == prototype(name.replace("_masked", ""))
    # SqairCarry itself did not change
    assert [n for n, _ in _capi.SqairCarry._fields_] == ["state_in", "state_out", "src_rows", "state_bytes", "B", "smc"]
    assert C.sizeof(_capi.SqairCarry) == 48
    # the one definition of the semantics sits above the calls
    phrases(paragraph("training on gappy and ragged streams: a per-frame", "int sqair_forward_train_carry_masked"),
            ("DRAWN FROM p_theta", "LATER IN THE SAME", "log_weights_per_timestep = 0", "exactly zero", "s / T'", "NULL observed",
             "T' + 1 kernel nodes"))
    # sqair_set_observed keeps refusing training calls, and its text points here
    doc = paragraph("missing-frame steps", "int sqair_set_observed")
    assert "out of scope" in doc and "sqair_forward_train_carry_masked" in doc


@pytest.mark.parametrize("path,flags", [
    (None, dict(k_particles=2, n_steps_per_image=3)),
    (_capi.WIDE_LIB_PATH, dict(k_particles=2, n_steps_per_image=3, n_what=64))])
@pytest.mark.parametrize("mask", [DUMMY, None])
def test_refusals_before_any_hip_call(path, flags, mask):
    """Everything the unmasked carried calls refuse, with a mask and with NULL for one, under the masked calls' names."""
    with handle(path, **flags) as (lib, h):
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
        refused(_carry(lib, h, smc=train_smc(ess_frac=0.5)), ["ess_frac"])       # adaptive-ESS training stays out of scope
        refused(_carry(lib, h, smc=train_smc(ess_frac=0.0)), ["ess_frac"])
        for k in ("log_w", "log_z", "log_evidence", "ess", "resampled", "src_rows"):
            refused(_carry(lib, h, smc=train_smc(**{k: None})), ["NULL"])
        refused(_carry(lib, h, smc=train_smc(src_rows=OTHER.value)), ["src_rows"])
        f, fe, g, ge = _calls(lib, h, _carry(lib, h, smc=train_smc()), lw=False, mask=mask)
        assert f == -1 and "log_weights_per_timestep" in fe
        # a handle that carries an inference state, with or without its own mask: the registrations never mix
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        refused(_carry(lib, h), ["sqair_set_state"])
        assert lib.sqair_set_observed(h, DUMMY, 2, B) == 0
        f, fe, g, ge = _calls(lib, h, _carry(lib, h), mask=mask)
        assert f == -1 and g == -1 and "sqair_set_observed" in fe and "sqair_set_observed" in ge
        # ... and the handle's mask keeps refusing the unmasked training calls (tests/test_missing_host.py pins the text)
        assert lib.sqair_forward_train(*fwd_args(h, B, T=2)) == -1
        assert "out of scope" in _err(lib, h)
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0


def test_refused_with_sample_from_prior_and_for_frames_too_large_to_train():
    with handle(k_particles=2, n_steps_per_image=3, sample_from_prior=True, generate_after=2) as (lib, h):
        f, fe, g, ge = _calls(lib, h, _carry(lib, h))
        assert f == -1 and g == -1 and "sample_from_prior" in fe and "sample_from_prior" in ge
    with handle(hw=(256, 256), k_particles=2, n_steps_per_image=3) as (lib, h):
        f, fe, g, ge = _calls(lib, h, _carry(lib, h))
        assert f == -1 and g == -1 and "training is limited" in fe and "training is limited" in ge


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
