"""-m gpu: a bounded part of the randomised dense sweep of tests/fuzz_linear.py -- 24 drawn shapes through sqair_linear_test and 6
drawn snt.GRU steps through sqair_gru_test against float64, at the script's own bars.  The seed is fixed here, one stream per case; rows are capped at
8192 for time (the script itself draws up to 30000)."""
import ctypes as C

import numpy as np
import pytest

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import make_config
from tests import fuzz_linear
from tests.hip_util import stream

pytestmark = pytest.mark.gpu

SEED, MAX_ROWS = 20250607, 8192


@pytest.fixture(scope="module")
def handle():
    lib = _capi.lib()
    cfg = make_config(make_flags(), (50, 50))
    h = C.c_void_p()
    assert lib.sqair_create(C.byref(cfg), C.byref(h)) == 0
    yield lib, h
    lib.sqair_destroy(h)


@pytest.mark.parametrize("i", range(24))
def test_drawn_shape(handle, i):
    lib, h = handle
    ok, err, bar = fuzz_linear.linear_shape(np.random.default_rng([SEED, i]), lib, h, stream(), max_rows=MAX_ROWS)
    assert ok, (err, bar)


@pytest.mark.parametrize("i", range(6))
def test_drawn_gru_step(handle, i):
    lib, h = handle
    ok, err, bar = fuzz_linear.gru_step(np.random.default_rng([SEED, 100 + i]), lib, h, stream(), max_rows=MAX_ROWS)
    assert ok, (err, bar)
