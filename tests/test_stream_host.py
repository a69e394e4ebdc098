"""Carried model state (include/sqair_hip.h: sqair_state_bytes / sqair_set_state), host side: the symbols, the blob size, and
every refusal -- all of them are decided before any HIP call, so dummy device pointers are enough and no GPU is needed."""
import ctypes as C
import os
import re

import pytest

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config

NEW = ("sqair_state_bytes", "sqair_set_state")
DUMMY = C.c_void_p(0x1000)     # never dereferenced: the calls below are refused first
BIG = 1 << 40


def _handle(path=None, hw=(50, 50), **flags):
    lib = _capi.lib(path)
    cfg = make_config(make_flags(**flags), hw)
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    return lib, h


def _err(lib, h):
    return lib.sqair_last_error(h).decode()


def test_state_symbols_are_exported_and_declared(repo_root):
    txt = open(os.path.join(repo_root, "include", "sqair_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = _capi.lib()
    for n in NEW:
        assert re.search(r"\b" + n + r"\s*\(", txt), n
        assert n in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, n)
    assert lib.sqair_abi_version() == 2


@pytest.mark.parametrize("path,flags", [
    (None, dict(k_particles=5, n_steps_per_image=4)),
    (None, dict(k_particles=2, n_steps_per_image=3, time_transition="LSTM", prior_transition="LSTM")),
    (None, dict(k_particles=3, n_steps_per_image=3, n_units=5)),
    (_capi.WIDE_LIB_PATH, dict(k_particles=2, n_steps_per_image=3, n_what=64))])
def test_state_bytes_positive_and_linear_in_B(path, flags):
    lib, h = _handle(path, **flags)
    try:
        b1 = lib.sqair_state_bytes(h, 1)
        assert b1 > 0 and b1 % (16 * int(flags["k_particles"])) == 0   # whole 16-byte rows, one per particle
        for B in (2, 7, 32):
            assert lib.sqair_state_bytes(h, B) == B * b1
        assert lib.sqair_state_bytes(h, 0) < 0
        # at least the records, both cell states, last id and counter of every slot row
        N = int(flags["n_steps_per_image"])
        assert b1 // int(flags["k_particles"]) >= 4 * (N * (2 * 32 * int(flags.get("n_units", 8))) + 2)
    finally:
        lib.sqair_destroy(h)


def test_wide_blob_differs_from_product_blob():
    """The blob is tied to the build: the wide library's slot record is larger."""
    lp, hp = _handle(None, k_particles=2, n_steps_per_image=3)
    lw, hw_ = _handle(_capi.WIDE_LIB_PATH, k_particles=2, n_steps_per_image=3)
    try:
        assert lw.sqair_state_bytes(hw_, 4) > lp.sqair_state_bytes(hp, 4)
    finally:
        lp.sqair_destroy(hp)
        lw.sqair_destroy(hw_)


def _fwd_args(h, B, t_offset=0, T=2):
    out = _capi.SqairOutputs()
    return (h, DUMMY, DUMMY, DUMMY, DUMMY, T, B, t_offset, C.byref(out), DUMMY, BIG, DUMMY)


def test_set_state_refusals():
    lib, h = _handle(k_particles=2, n_steps_per_image=3)
    try:
        need = lib.sqair_state_bytes(h, 4)
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, need - 4, 4) == -1
        assert "state_bytes" in _err(lib, h)
        assert lib.sqair_set_state(h, None, None, DUMMY, need, 4) == -1     # a source map without a blob to map
        assert "state_in" in _err(lib, h)
        assert lib.sqair_set_state(h, None, DUMMY, DUMMY, need, 4) == -1
        assert lib.sqair_set_state(h, DUMMY, DUMMY, DUMMY, need, 4) == 0
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0          # all NULL: off
    finally:
        lib.sqair_destroy(h)
    lib, h = _handle(k_particles=2, n_steps_per_image=3, sample_from_prior=True, generate_after=2)
    try:
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, BIG, 4) == -1
        assert "sample_from_prior" in _err(lib, h)
    finally:
        lib.sqair_destroy(h)


def test_passes_refused_while_a_state_is_set():
    lib, h = _handle(k_particles=2, n_steps_per_image=3)
    try:
        B = 4
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        # training / backward with a carried state
        assert lib.sqair_forward_train(*_fwd_args(h, B)) == -1
        assert "training" in _err(lib, h)
        assert lib.sqair_backward(h, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, DUMMY, 2, B, 0, DUMMY, BIG, DUMMY, BIG, DUMMY, DUMMY) == -1
        assert "training" in _err(lib, h)
        # t_offset with state_in: the counter is the time index
        for fn in (lib.sqair_forward, lib.sqair_graph_capture):
            assert fn(*_fwd_args(h, B, t_offset=3)) == -1
            assert "t_offset" in _err(lib, h)
            # B other than the state's
            assert fn(*_fwd_args(h, B + 1)) == -1
            assert "B = 5" in _err(lib, h)
        # export only (state_in NULL): t_offset is allowed, B is still checked
        assert lib.sqair_set_state(h, None, DUMMY, None, lib.sqair_state_bytes(h, B), B) == 0
        assert lib.sqair_forward(*_fwd_args(h, B - 1, t_offset=3)) == -1
        assert "B = 3" in _err(lib, h)
    finally:
        lib.sqair_destroy(h)
