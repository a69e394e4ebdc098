"""-m gpu: the object-layers kernel (k_lane_layers, through sqair_lane_layers_test) against the float64 reference of
tests/layers_ref.py, on caller buffers, for the cases of tests/layers_cases.py: K in {1, 2, 3, 5, 64, 65, 256} (one wave, a wave
boundary, every thread of the workgroup), T = 3 for the prefix weights, 50 x 50 frames, 12 x 9 frames whose boxes are larger than
the frame, a 10 x 130 frame (wider than a wavefront), a 70 x 70 frame (several pixel tiles, H * W a multiple of nothing) and N = 14 on
the wide library, 11 to 48 lanes each, the last three non-finite.

``match`` is compared exactly with the reference's, except for the decisions tests/estimate_check.py's rule puts within 1e-5 of a
threshold: those are skipped and counted, at most 1 % of the decisions (tests/test_layers_ref.py holds the same inputs to that cap
from the reference alone).  ``layer`` and ``cover`` are compared against the reference evaluated with the device's OWN match table,
so that no threshold enters the pixel values and nothing is skipped: 2e-5 absolute, the decoder's own gate in
tests/test_hip_kernels.py::test_st_insert_loglik at the same glimpse magnitude (0.3 N(0, 1)) -- the outputs are convex combinations of
the quantities that test bounds.  ``owner`` is compared exactly against the owner rule applied to the device's own ``cover``.
Non-finite lanes give NaN and -1, absent objects zeros, and each optional pointer may be NULL without changing the others' bits.
With SQAIR_PARITY_DIR set the largest observed errors are written to layers_parity.json there (the copy under profiles/ is such a
file); without it nothing is written."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import layers_cases as LC
from tests import layers_ref as L
from tests.abi_host import open_handle
from tests.kernel_unit import merge_parity

pytestmark = pytest.mark.gpu

FIELDS = ("match", "layer", "cover", "owner")
NOTE = ("largest absolute error of layer and cover against the float64 reference evaluated with the device's own match "
        "table, per case of tests/test_layers_kernel.py (allowed: {:g}); match decisions skipped within 1e-5 of a "
        "threshold".format(LC.TOL))


def _record(case, **figures):
    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data["cases"][case] = figures
    merge_parity("layers_parity.json", lambda: {"note": NOTE, "cases": {}}, update)


_handles = {}


def _handle(c):
    key = (c.wide, c.N, c.hw, c.G)
    if key not in _handles:
        _handles[key] = open_handle(_capi.WIDE_LIB_PATH if c.wide else None, c.hw, k_particles=2, n_steps_per_image=c.N, n_what=6,
                                    glimpse_size=c.G)
    return _handles[key]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """The case's inputs, on the host and on the device, and the reference with its own match table: made once, never written to."""
    c = LC.CASES[i]
    x = LC.make(c)
    dev = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32).cuda()
    d = {k: dev(x[k]) for k in ("glimpse", "where", "presence", "lw", "lw0")}
    ref = L.layers(x["glimpse"], x["where"], x["presence"], x["lw"], c.K, c.hw, LC.IOU_MIN, LC.COVER_MIN, lw0=x["lw0"])
    return x, d, ref


def _run(c, d, B, fields=FIELDS, log_w=True, cover_min=LC.COVER_MIN):
    lib, h = _handle(c)
    shapes = _capi.layers_shapes(c.T, B, c.K, c.N, c.hw)
    o = {n: torch.full(shapes[n], -7, dtype=torch.int32 if n in _capi.LAYERS_INT_FIELDS else torch.float32, device="cuda") for n in fields}
    lay = _capi.SqairLaneLayers(cover_min=cover_min, **{n: t.data_ptr() for n, t in o.items()})
    s = torch.cuda.current_stream()
    rc = lib.sqair_lane_layers_test(h, d["glimpse"].data_ptr(), d["where"].data_ptr(), d["presence"].data_ptr(), d["lw"].data_ptr(),
                                    d["lw0"].data_ptr() if log_w else None, LC.IOU_MIN, c.T, B, c.K, C.byref(lay),
                                    C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("i", range(len(LC.CASES)), ids=[LC.case_id(c) for c in LC.CASES])
def test_layers_kernel_against_fp64(i):
    c = LC.CASES[i]
    x, d, ref = _inputs(i)
    B = x["B"]
    got = _run(c, d, B)
    fin, bad = ~ref.bad, ref.bad
    # ---- match: exact, but for the decisions within 1e-5 of a threshold
    near, decisions = L.near_decisions(ref.est, LC.IOU_MIN)
    differ = got["match"] != ref.match
    print(LC.case_id(c), "decisions", decisions, "near a threshold", int(near.sum()), "of which the device decided otherwise", int((differ & near).sum()))
    assert decisions > 0 and near.sum() <= 0.01 * decisions
    assert not (differ & ~near).any(), np.argwhere(differ & ~near)[:4]
    assert (got["match"][bad] == -1).all() and (got["match"][~np.broadcast_to(ref.present[:, :, None, :], differ.shape)] == -1).all()
    assert (got["match"] >= 0).any() and (c.K == 1 or (got["match"][np.broadcast_to((ref.present & fin[..., None])[:, :, None, :], differ.shape)] == -1).any())
    # ---- layer and cover: against the reference evaluated with the device's own match table
    own = L.layers(x["glimpse"], x["where"], x["presence"], x["lw"], c.K, c.hw, LC.IOU_MIN, LC.COVER_MIN, lw0=x["lw0"], match=got["match"])
    worst = {}
    for name in ("layer", "cover"):
        g, r = got[name], getattr(own, name)
        assert np.isnan(g[bad]).all() and np.isfinite(g[fin]).all(), name
        assert not _bits(g[fin][~ref.present[fin]]).any(), name                  # absent objects: zeros
        worst[name] = float(np.abs(g[fin].astype(np.float64) - r[fin]).max())
    print(LC.case_id(c), "largest error: layer {:.3g}, cover {:.3g}; allowed {:g}".format(worst["layer"], worst["cover"], LC.TOL))
    _record(LC.case_id(c), layer=worst["layer"], cover=worst["cover"], decisions=decisions, near=int(near.sum()),
            differing=int((differ & near).sum()), lanes=B)
    assert worst["layer"] <= LC.TOL and worst["cover"] <= LC.TOL, worst
    assert np.abs(got["layer"][fin]).max() > 0.1 and got["cover"][fin].max() > 0.9           # (something was drawn)
    # ---- owner: the rule on the device's own cover, exactly
    want = np.where(bad[:, :, None, None], -1, L.owner_rule(got["cover"], ref.present, LC.COVER_MIN))
    assert np.array_equal(got["owner"], want), np.argwhere(got["owner"] != want)[:4]
    assert (got["owner"][fin] >= 0).any() and (got["owner"][fin] == -1).any() and (got["owner"][bad] == -1).all()


@pytest.mark.parametrize("i", [2, 7, 8], ids=[LC.case_id(LC.CASES[i]) for i in (2, 7, 8)])
def test_each_optional_pointer_may_be_null(i):
    """Any subset of the four outputs gives the bits of the full run; a NULL log_w means zeros; cover_min moves owner alone."""
    c = LC.CASES[i]
    x, d, _ = _inputs(i)
    B = x["B"]
    full = _run(c, d, B)
    for fields in (("match",), ("layer",), ("cover",), ("owner",), ("layer", "owner"), ("match", "cover")):
        part = _run(c, d, B, fields=fields)
        for n in fields:
            assert np.array_equal(_bits(part[n]), _bits(full[n])), (fields, n)
    zero = dict(d, lw0=torch.zeros_like(d["lw0"]))
    a, b = _run(c, zero, B), _run(c, d, B, log_w=False)
    for n in FIELDS:
        assert np.array_equal(_bits(a[n]), _bits(b[n])), n
    low = _run(c, d, B, cover_min=0.25)
    for n in ("match", "layer", "cover"):
        assert np.array_equal(_bits(low[n]), _bits(full[n])), n
    assert ((low["owner"] >= 0) & (full["owner"] == -1)).any() and not ((low["owner"] == -1) & (full["owner"] >= 0)).any()
