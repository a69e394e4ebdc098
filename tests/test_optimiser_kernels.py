"""-m gpu: the optimiser and debug kernels k_rmsprop, k_add_l2 and k_finite_check, each on its own through the product's entries
(sqair_rmsprop_step, sqair_add_l2_grad, sqair_check_finite).

k_rmsprop.  n 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 3 x 1024 + 1, each with all four buffers 16-byte aligned (the float4 path) and with
one of theta, grad, ms, mom starting one word later (which puts the whole launch on the scalar path; n = 3 and n = 1025 with each
of the four in turn); ms from {0, 1e-12, 1, 1e6} per
element, g = N(0, 1) x 10^U(-4, 2) with exact zeros (ms = 0 with g = 0 gives 0 / sqrt(eps) = 0, not NaN), mom mixed; grad_scale 1,
0.5, 0.125; the default hyper-parameters and (lr 3e-2, decay 0.95, momentum 0, eps 1e-6).  One step from the given float32 state is
judged per element against sqair_amd.train.rmsprop_reference in float64: theta's error divided by max(|theta|, |mom|, lr), ms and
mom relative; three consecutive steps against the reference carrying its own float64 state.  grad is unchanged bit for bit, and so
are the guard words before element 0 and after element n - 1 of all four buffers.  Whether the float4 and the scalar path agree bit
for bit is recorded in the parity file, not asserted: the compiler may contract them differently.

k_add_l2.  n 1, 255, 256, 257, 70001, grad of mixed magnitude, l2 1e-4 and 0.5, against grad + l2 theta in float64, relative to
|grad| + l2 |theta|; l2 = 0 and n = 0 return 0 and leave grad as it was; theta and the guard words unchanged.

k_finite_check.  Integer-exact: count and first index as parsed out of sqair_last_error, and as flag_dev holds them, equal NumPy's.
The clamp of the first index to 0x7fffffff beyond 2^31 elements is not tested.

The bars are 8 x the worst error of the same formulas in float32 over a kernel's cases (tests/objective_ref.py; the power check of
tests/test_objective_ref.py makes five mistakes in them and these cases see each).  With SQAIR_PARITY_DIR set the figures go to
objective_parity.json beside those of tests/test_objective_kernels.py."""
import re

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import kernel_unit as U
from tests import objective_ref as OR
from tests import slot_adjoint_ref as R
from tests.hip_util import stream
from tests.kernel_unit import F32, F64, Buf

pytestmark = pytest.mark.gpu

GUARD = 8                      # words before element 0 (a multiple of 4: the data stays 16-byte aligned) and after element n - 1
NOTE = OR.PARITY_NOTE
PARITY = U.Parity(OR.PARITY_FILE, NOTE, worst_ratio=True)
RMS_CASES = OR.rms_cases()
_agree = {}                    # k_rmsprop: {n: do the float4 path and the scalar path give the same bits}
_worst = U.Cases(lambda key: OR.rms_worst32() if key == "k_rmsprop" else (dict(grad=OR.l2_worst32()) if key == "k_add_l2" else _three32()))


def handle():
    return U.handle("objective K5", lambda name: U.Handle(name, False, (50, 50), 3, 5, {}))


def worst32(kernel):
    return _worst(kernel)


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    U.close()
    PARITY.write(worst32)
    if _agree:
        U.merge_parity(PARITY.file_name, lambda: {"note": NOTE, "build_id": _capi.build_id(), "bars": {}, "cases": {}, "worst_ratio": {}},
                       lambda data: data.update(k_rmsprop_float4_and_scalar_paths_agree_bitwise={str(n): v for n, v in sorted(_agree.items())}))


def guarded(data, start, shift=0, owned=True):
    """(Buf, pointer of element 0): `data` between GUARD (+ shift) and GUARD distinct sentinel words."""
    data = np.asarray(data, F32)
    n, first = data.size, GUARD + shift
    host = R.distinct_words(first + n + GUARD, start).copy()
    host[first:first + n] = data
    own = np.zeros(host.shape, bool)
    own[first:first + n] = owned
    b = Buf(host, own)
    assert b.t.data_ptr() % 16 == 0
    return b, b.ptr(first), slice(first, first + n)


def _rms_launch(hd, state, hyper, gs, off=None, steps=None):
    """One step (or one per gradient of `steps`) on guarded buffers, the buffer named `off` one word off: (theta, ms, mom)."""
    theta, g, ms, mom = state
    names = ("theta", "grad", "ms", "mom")
    bufs = {k: guarded(v, i << 16, int(k == off), owned=k != "grad") for i, (k, v) in enumerate(zip(names, (theta, g, ms, mom)))}
    misaligned = [k for k in names if bufs[k][1] % 16]
    assert misaligned == ([] if off in (None, "aligned") else [off])
    for grad in (steps or [g]):
        bufs["grad"][0].t[bufs["grad"][2]] = torch.from_numpy(np.asarray(grad, F32)).cuda()
        bufs["grad"][0].before[bufs["grad"][2]] = grad
        hd.check(hd.lib.sqair_rmsprop_step(hd.h, bufs["theta"][1], bufs["grad"][1], bufs["ms"][1], bufs["mom"][1], len(theta), hyper["lr"],
                                           hyper["decay"], hyper["momentum"], hyper["eps"], gs, stream()), "sqair_rmsprop_step")
    for k in names:
        bufs[k][0].check_untouched(k)                                   # grad: every word; the others: their guard words
    return tuple(bufs[k][0].after()[bufs[k][2]] for k in ("theta", "ms", "mom"))


@pytest.mark.parametrize("case", list(RMS_CASES))
def test_rmsprop_one_step(case):
    n, off, hyper, gs = RMS_CASES[case]
    state = OR.rms_state(n, list(RMS_CASES).index(case))
    got = _rms_launch(handle(), state, hyper, gs, off)
    ref = OR.rms_step(*state, hyper, gs)
    assert np.isfinite(np.concatenate(got)).all()
    e = OR.rms_errors(got, ref, state, hyper)
    e32 = OR.rms_errors(OR.rms_step(*state, hyper, gs, dt=F32), ref, state, hyper)
    if off != "aligned":                                              # the same launch on the float4 path: recorded, not asserted
        vec = _rms_launch(handle(), state, hyper, gs, "aligned")
        _agree[n] = _agree.get(n, True) and bool(all(np.array_equal(U.bits(a), U.bits(b)) for a, b in zip(got, vec)))
    U.judge(PARITY, "k_rmsprop", case, e, e.get, e32, worst32("k_rmsprop"))


THREE = (1025, 77, OR.RMS_HYPER[0], 0.5)


def _three32():
    (ref, _), (r32, _) = OR.rms_three_steps(*THREE, dt=F64), OR.rms_three_steps(*THREE, dt=F32)
    return OR.rms_errors(r32, ref, OR.rms_state(*THREE[:2]), THREE[2])


@pytest.mark.parametrize("off", ["aligned", "ms"])
def test_rmsprop_three_steps(off):
    """Three consecutive steps (as if summed over two ranks: grad_scale 0.5) against the reference carrying its own float64 state."""
    n, seed, hyper, gs = THREE
    ref, grads = OR.rms_three_steps(n, seed, hyper, gs, F64)
    state = OR.rms_state(n, seed)
    got = _rms_launch(handle(), state, hyper, gs, off, steps=grads)
    e = OR.rms_errors(got, ref, state, hyper)
    U.judge(PARITY, "k_rmsprop x3", "n%d %s" % (n, off), e, e.get, _three32(), worst32("k_rmsprop x3"))


@pytest.mark.parametrize("l2", OR.L2_WEIGHTS)
@pytest.mark.parametrize("n", OR.L2_N)
def test_add_l2(n, l2):
    hd = handle()
    theta, grad = OR.l2_state(n, OR.L2_N.index(n))
    (bt, pt, _), (bg, pg, sg) = guarded(theta, 0, owned=False), guarded(grad, 1 << 20)
    hd.check(hd.lib.sqair_add_l2_grad(hd.h, pt, pg, n, l2, stream()), "sqair_add_l2_grad")
    bt.check_untouched("theta"); bg.check_untouched("grad")
    got = bg.after()[sg]
    e = dict(grad=OR.l2_error(got, theta, grad, l2))
    U.judge(PARITY, "k_add_l2", "n%d l2 %g" % (n, l2), e, e.get, dict(grad=OR.l2_error(OR.l2_step(theta, grad, l2, dt=F32), theta, grad, l2)),
            worst32("k_add_l2"))


def test_add_l2_nothing_to_add():
    hd = handle()
    theta, grad = OR.l2_state(257, 9)
    (bt, pt, _), (bg, pg, _) = guarded(theta, 0, owned=False), guarded(grad, 1 << 20, owned=False)
    assert hd.lib.sqair_add_l2_grad(hd.h, pt, pg, 257, 0.0, stream()) == 0 and hd.lib.sqair_add_l2_grad(hd.h, pt, pg, 0, 0.5, stream()) == 0
    bt.check_untouched("theta"); bg.check_untouched("grad")


# ------------------------------------------------------------------------------------------------ k_finite_check
MESSAGE = re.compile(r"^non-finite values in (.*): (\d+) of (\d+), first at flat index (\d+)$")


def _finite(hd, x, what=b"the tensor under test"):
    """sqair_check_finite on x between NaN guard words: (return code, (count, first) parsed from the error text or None, flag_dev)."""
    x = np.asarray(x, F32)
    host = np.full(GUARD + x.size + GUARD, np.nan, F32)
    host[GUARD:GUARD + x.size] = x
    bx = Buf(host)
    flag = Buf(np.array([11, 12, 13, 14, 15, 16], np.int32), np.array([0, 0, 1, 1, 0, 0], bool))
    rc = hd.lib.sqair_check_finite(hd.h, bx.ptr(GUARD), x.size, what, flag.ptr(2), stream())
    bx.check_untouched("x"); flag.check_untouched("flag_dev")
    m = MESSAGE.match(hd.lib.sqair_last_error(hd.h).decode()) if rc != 0 else None
    if m:
        assert m.group(1) == what.decode() and int(m.group(3)) == x.size
    return rc, (int(m.group(2)), int(m.group(4))) if m else None, tuple(int(v) for v in flag.after()[2:4])


def _clean(rng, n):
    """Everything a finite check must let through: +-FLT_MAX, denormals, +-0 and ordinary values."""
    special = np.array([np.finfo(F32).max, -np.finfo(F32).max, 1e-45, -1e-45, 1e-39, np.finfo(F32).tiny, 0.0, -0.0], F32)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(F32)
    at = rng.uniform(size=n) < 0.3
    x[at] = rng.choice(special, int(at.sum()))
    x[:min(n, special.size)] = special[:min(n, special.size)]
    assert np.isfinite(x).all()
    return x


def test_finite_check():
    hd, rng = handle(), np.random.default_rng(3)
    assert _finite(hd, _clean(rng, 5000)) == (0, None, (0, 0x7fffffff))
    assert _finite(hd, np.zeros(0, F32)) == (0, None, (0, 0x7fffffff))                       # n = 0
    for bad in (np.nan, np.inf, -np.inf):
        for n, at in ((1, 0), (777, 0), (777, 776), (1024 * 256 + 300, 1024 * 256 + 299)):
            x = _clean(rng, n)
            x[at] = bad
            assert _finite(hd, x) == (-5, (1, at), (1, at)), (bad, n, at)
        assert _finite(hd, _clean(rng, 300)) == (0, None, (0, 0x7fffffff))                   # the handle keeps working
    n = 1024 * 256 + 300                                                                     # the last one sits in the grid-stride second round
    x = _clean(rng, n)
    x[5], x[n - 1] = np.inf, np.nan
    assert _finite(hd, x) == (-5, (2, 5), (2, 5))
    x = _clean(rng, n)
    at = rng.permutation(n)[:1000]
    x[at] = rng.choice(np.array([np.nan, np.inf, -np.inf], F32), 1000)
    want = (int((~np.isfinite(x)).sum()), int(np.argmax(~np.isfinite(x))))
    assert want == (1000, int(at.min())) and _finite(hd, x) == (-5, want, want)
    assert _finite(hd, _clean(rng, n)) == (0, None, (0, 0x7fffffff))
