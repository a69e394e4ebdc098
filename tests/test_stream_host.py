"""Carried model state (include/sqair_hip.h: sqair_state_bytes / sqair_set_state), host side: the symbols, the blob size, and
every refusal -- all of them are decided before any HIP call, so dummy device pointers are enough and no GPU is needed."""
import functools

import pytest

from sqair_amd import _capi
from tests.abi_host import BIG, DUMMY, err as _err, functions, fwd_args, handle

NEW = ("sqair_state_bytes", "sqair_set_state")


def test_state_symbols_are_exported_and_declared():
    lib = _capi.lib()
    for n in NEW:
        assert n in functions(), n
        assert n in _capi.EXPORTED_SYMBOLS
        assert hasattr(lib, n)
    assert lib.sqair_abi_version() == 2


@pytest.mark.parametrize("path,flags", [
    (None, dict(k_particles=5, n_steps_per_image=4)),
    (None, dict(k_particles=2, n_steps_per_image=3, time_transition="LSTM", prior_transition="LSTM")),
    (None, dict(k_particles=3, n_steps_per_image=3, n_units=5)),
    (_capi.WIDE_LIB_PATH, dict(k_particles=2, n_steps_per_image=3, n_what=64))])
def test_state_bytes_positive_and_linear_in_B(path, flags):
    with handle(path, **flags) as (lib, h):
        b1 = lib.sqair_state_bytes(h, 1)
        assert b1 > 0 and b1 % (16 * int(flags["k_particles"])) == 0   # whole 16-byte rows, one per particle
        for B in (2, 7, 32):
            assert lib.sqair_state_bytes(h, B) == B * b1
        assert lib.sqair_state_bytes(h, 0) < 0
        # at least the records, both cell states, last id and counter of every slot row
        N = int(flags["n_steps_per_image"])
        assert b1 // int(flags["k_particles"]) >= 4 * (N * (2 * 32 * int(flags.get("n_units", 8))) + 2)


def test_wide_blob_differs_from_product_blob():
    """The blob is tied to the build: the wide library's slot record is larger."""
    flags = dict(k_particles=2, n_steps_per_image=3)
    with handle(None, **flags) as (lp, hp), handle(_capi.WIDE_LIB_PATH, **flags) as (lw, hw_):
        assert lw.sqair_state_bytes(hw_, 4) > lp.sqair_state_bytes(hp, 4)


_fwd_args = functools.partial(fwd_args, T=2, bind=())


def test_set_state_refusals():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
        need = lib.sqair_state_bytes(h, 4)
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, need - 4, 4) == -1
        assert "state_bytes" in _err(lib, h)
        assert lib.sqair_set_state(h, None, None, DUMMY, need, 4) == -1     # a source map without a blob to map
        assert "state_in" in _err(lib, h)
        assert lib.sqair_set_state(h, None, DUMMY, DUMMY, need, 4) == -1
        assert lib.sqair_set_state(h, DUMMY, DUMMY, DUMMY, need, 4) == 0
        assert lib.sqair_set_state(h, None, None, None, 0, 0) == 0          # all NULL: off
    with handle(k_particles=2, n_steps_per_image=3, sample_from_prior=True, generate_after=2) as (lib, h):
        assert lib.sqair_set_state(h, DUMMY, DUMMY, None, BIG, 4) == -1
        assert "sample_from_prior" in _err(lib, h)


def test_passes_refused_while_a_state_is_set():
    with handle(k_particles=2, n_steps_per_image=3) as (lib, h):
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
