"""No GPU: the C-ABI of the missing-frame steps (include/sqair_hip.h: sqair_set_observed) -- exported and declared, every refusal
made before any HIP call (dummy device pointers are enough) -- and the argument errors of SqairStream(missing=...).step(observed=...)."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests.abi_host import (BIG, DUMMY, LIBS, constant, err as _err, fwd_args as _fwd_args, handle, paragraph, phrases, prototype,
                            set_state as _state)


def test_the_symbol_is_exported_and_declared_and_the_abi_is_unchanged():
    for path in LIBS:
        lib = _capi.lib(path)
        assert hasattr(lib, "sqair_set_observed") and lib.sqair_abi_version() == 2
    assert "sqair_set_observed" in _capi.EXPORTED_SYMBOLS
    assert prototype("sqair_set_observed") == "int sqair_set_observed(SqairHandle* h, const int32_t* observed, int T, int B)"
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    # the one definition of the semantics sits above the call, and says that training on gappy streams is out of scope
    phrases(paragraph("missing-frame steps", "int sqair_set_observed"),
            ("HELD", "log_weights_per_timestep = 0", "FINITE", "T + 1 kernel nodes", "out of scope"))


def test_set_observed_refusals_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        assert lib.sqair_set_observed(None, DUMMY, 1, B) == -1
        assert lib.sqair_set_observed(h, DUMMY, 1, B) == -1 and "carried state" in _err(lib, h)      # no state set
        _state(lib, h, B)
        for T in (0, -3):
            assert lib.sqair_set_observed(h, DUMMY, T, B) == -1 and "T must be >= 1" in _err(lib, h)
        assert lib.sqair_set_observed(h, DUMMY, 1, B + 1) == -1 and "B = 5" in _err(lib, h) and "B = 4" in _err(lib, h)
        assert lib.sqair_set_observed(h, DUMMY, 3, B) == 0
        assert lib.sqair_set_observed(h, None, 0, 0) == 0        # NULL: off
        # off: a pass of another T gets past the mask's check (B + 1 stops it at the state's)
        assert lib.sqair_forward(*_fwd_args(h, B + 1, T=2)) == -1 and "observed" not in _err(lib, h)
    with handle(k_particles=2, n_steps_per_image=3, sample_from_prior=True) as (lib, h):
        assert lib.sqair_set_observed(h, DUMMY, 1, 4) == -1 and "sample_from_prior" in _err(lib, h)


def test_pass_time_refusals_before_any_hip_call():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        _state(lib, h, B)
        assert lib.sqair_set_observed(h, DUMMY, 2, B) == 0
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            for T in (1, 3):   # a pass whose T is not the registered one
                assert fn(*_fwd_args(h, B, T=T)) == -1
                assert "sqair_set_observed" in _err(lib, h) and "T = 2" in _err(lib, h) and "T = {}".format(T) in _err(lib, h)
        # every training call while a mask is set: training on gappy streams is out of scope, and the text says so
        assert lib.sqair_forward_train(*_fwd_args(h, B, T=2)) == -1
        assert "sqair_set_observed" in _err(lib, h) and "out of scope" in _err(lib, h)
        carry = _capi.SqairCarry(state_in=0x1000, state_out=0x1000, src_rows=None, state_bytes=lib.sqair_state_bytes(h, B), B=B, smc=None)
        out = _capi.SqairOutputs(log_weights_per_timestep=0x1000)
        assert lib.sqair_forward_train_carry(h, DUMMY, DUMMY, DUMMY, DUMMY, 2, B, C.byref(carry), C.byref(out), DUMMY, BIG, DUMMY) == -1
        assert "sqair_set_observed" in _err(lib, h) and "out of scope" in _err(lib, h)


def test_the_state_going_off_or_to_another_b_takes_the_mask_with_it():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        B = 4
        mask_refuses = lambda T: lib.sqair_forward(*_fwd_args(h, B, T=T)) == -1 and "sqair_set_observed" in _err(lib, h)
        _state(lib, h, B)
        assert lib.sqair_set_observed(h, DUMMY, 2, B) == 0
        assert mask_refuses(3)
        _state(lib, h, B)                  # the same B again: the mask stays
        assert mask_refuses(3)
        # (every pass below is still refused on the host, by a check that comes AFTER the mask's: a wrong B for the state)
        other_b_refuses = lambda: (lib.sqair_forward(*_fwd_args(h, B + 7, T=3)) == -1 and "sqair_set_observed" not in _err(lib, h) and
                                   "B = {}".format(B + 7) in _err(lib, h))
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0
        _state(lib, h, B)                  # the state off and on again: the mask is gone
        assert other_b_refuses()
        assert lib.sqair_set_observed(h, DUMMY, 2, B) == 0
        _state(lib, h, B + 1)              # another B: off
        assert other_b_refuses()


def test_stream_argument_errors():
    """``observed`` is checked before the stream touches its core."""
    def stream(missing, T=1, B=3):
        st = SqairStream.__new__(SqairStream)
        st.missing, st.T, st.B = missing, T, B
        return st
    with pytest.raises(ValueError, match=r"^SqairStream.step: observed is for a stream with missing=True"):
        stream(False).step(None, observed=np.ones(3, bool))
    st = stream(True)
    assert st._check_observed(None) is None
    assert tuple(st._check_observed(np.array([True, False, True])).shape) == (1, 3)     # [B] when T' = 1
    assert torch.equal(st._check_observed([[True, False, True]]), torch.tensor([[True, False, True]]))
    for bad in (np.ones(4, bool), np.ones((2, 3), bool), np.ones((1, 3, 1), bool)):
        with pytest.raises(ValueError, match=r"^SqairStream.step: observed of shape .* \[1, 3\] expected \(or \[3\]\)"):
            st.step(None, observed=bad)
    for bad in (np.ones(3, np.int32), np.ones(3, np.float32)):
        with pytest.raises(ValueError, match=r"^SqairStream.step: observed must be a bool array"):
            st.step(None, observed=bad)
    st = stream(True, T=4)
    assert tuple(st._check_observed(np.ones((4, 3), bool)).shape) == (4, 3)
    with pytest.raises(ValueError, match=r"^SqairStream.step: observed of shape \(3,\) given, \[4, 3\] expected$"):
        st.step(None, observed=np.ones(3, bool))   # [B] alone is for one-frame steps
