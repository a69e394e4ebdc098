"""No GPU: the C-ABI of the missing-frame steps (include/sqair_hip.h: sqair_set_observed) -- exported and declared, every refusal
made before any HIP call (dummy device pointers are enough) -- and the argument errors of SqairStream(missing=...).step(observed=...)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from sqair_amd.stream import SqairStream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMMY = C.c_void_p(0x1000)     # never dereferenced: the calls below are refused first
BIG = 1 << 50


def _handle(path=None, hw=(50, 50), **flags):
    lib = _capi.lib(path)
    cfg = make_config(make_flags(**flags), hw)
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


def _err(lib, h):
    return lib.sqair_last_error(h).decode()


def _state(lib, h, B):
    assert lib.sqair_set_state(h, DUMMY, DUMMY, DUMMY, lib.sqair_state_bytes(h, B), B) == 0


def _fwd_args(h, B, T=1, bind=("log_weights_per_timestep",)):
    out = _capi.SqairOutputs(**{k: 0x1000 for k in bind})
    return (h, DUMMY, DUMMY, DUMMY, DUMMY, T, B, 0, C.byref(out), DUMMY, BIG, DUMMY)


def test_the_symbol_is_exported_and_declared_and_the_abi_is_unchanged():
    hdr = open(os.path.join(ROOT, "include", "sqair_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for path in (None, _capi.WIDE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, "sqair_set_observed") and lib.sqair_abi_version() == 2
    assert "sqair_set_observed" in _capi.EXPORTED_SYMBOLS
    assert re.search(r"\bint\s+sqair_set_observed\s*\(\s*SqairHandle\*\s*h,\s*const int32_t\*\s*observed\s*,\s*int T,\s*int B\)", code)
    assert _capi.ABI_VERSION == 2 and re.search(r"#define SQAIR_ABI_VERSION 2\b", hdr)
    # the one definition of the semantics sits above the call, and says that training on gappy streams is out of scope
    doc = hdr[hdr.index("missing-frame steps"):hdr.index("int sqair_set_observed")]
    for word in ("HELD", "log_weights_per_timestep = 0", "FINITE", "T + 1 kernel nodes", "out of scope"):
        assert word in doc, word


def test_set_observed_refusals_before_any_hip_call():
    lib, h = _handle(k_particles=2, n_steps_per_image=3)
    try:
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
    finally:
        lib.sqair_destroy(h)
    lib, h = _handle(k_particles=2, n_steps_per_image=3, sample_from_prior=True)
    try:
        assert lib.sqair_set_observed(h, DUMMY, 1, 4) == -1 and "sample_from_prior" in _err(lib, h)
    finally:
        lib.sqair_destroy(h)


def test_pass_time_refusals_before_any_hip_call():
    lib, h = _handle(k_particles=2, n_steps_per_image=3)
    try:
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
    finally:
        lib.sqair_destroy(h)


def test_the_state_going_off_or_to_another_b_takes_the_mask_with_it():
    lib, h = _handle(k_particles=2, n_steps_per_image=3)
    try:
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
    finally:
        lib.sqair_destroy(h)


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
