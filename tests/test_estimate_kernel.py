"""-m gpu: the lane-estimate kernel (k_lane_estimate, through sqair_lane_estimate_test) against the float64 reference of
tests/estimate_ref.py, on caller buffers: K in {1, 2, 5, 64, 65, 256} (one wave, a wave boundary, every thread of the workgroup),
T in {1, 3} (prefix weights), N = 4 on the product library and N = 14 on the wide one, 50 x 50 frames and a 12 x 9 case whose boxes
are larger than the frame, one to two hundred lanes per case.  (N = 14 is the most a handle takes: the wide build is compiled for 16
slots, but sqair_create refuses 15 and 16 -- the log-probability adjoint's LDS staging, tests/test_capi_host.py -- and the entry
point takes N from its handle.)

A lane's particles are jittered copies of a base scene (sigma 0.02 / 0.15 / 0.5 in logit units: all agree / the threshold cuts
through them / few agree) with random presence -- lanes without an object and lanes with all N among them -- and the weight patterns
of tests/test_smc_kernel.py (random, equal, dominant, spread, neg_inf), plus a NaN lane, a +inf lane and an all -inf lane.

The comparison and its tolerances are tests/estimate_check.py's: integer outputs and copied words exact, the weights and the sums
of weights within the fp32 rounding band of the header's fixed-order sums capped at 1e-5 relative, boxes within 16 * 2^-24 *
max(H, W) pixels, decisions inside 1e-5 of a threshold skipped and counted -- at most 1 % of them."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import estimate_check as EC
from tests import estimate_ref as E
from tests.abi_host import open_handle

pytestmark = pytest.mark.gpu

PATTERNS = ("random", "equal", "dominant", "spread", "neg_inf")
SIGMAS = (0.02, 0.15, 0.5)
N_WHAT = 6


def _lanes(K, T, N, per_cell, rng, big_boxes):
    """where [T, R, N, 4], presence, obj_id [T, R, N], what [T, R, N, N_WHAT], lw0 [R], lw [T, R] and the lanes' pattern names."""
    cells = [(p, s) for p in PATTERNS for s in SIGMAS]
    B = per_cell * len(cells) + 3
    sig = np.array([s for _, s in cells for _ in range(per_cell)] + [0.15] * 3)
    names = [p for p, _ in cells for _ in range(per_cell)] + ["nan", "pos_inf", "all_neg_inf"]
    base = rng.standard_normal((T, B, 1, N, 4))
    base[..., :2] = base[..., :2] * 0.7 + (3.0 if big_boxes else -1.0)   # the scale logits: boxes of ~1/4 of the frame, or beyond it
    where = (base + sig[None, :, None, None, None] * rng.standard_normal((T, B, K, N, 4))).astype(np.float32)
    n_obj = rng.integers(0, N + 1, size=(T, B))
    n_obj[:, 0::7] = 0          # lanes with no object in the base scene ...
    n_obj[:, 1::7] = N          # ... and with all N
    base_p = np.arange(N)[None, None, :] < n_obj[..., None]
    flip = rng.uniform(size=(T, B, K, N)) < 0.15                          # particles disagree on the count, holes included
    flip[:, 0::7] = False
    flip[:, 1::7] = False
    pres = (base_p[:, :, None, :] ^ flip).astype(np.float32)
    ids = rng.integers(0, 50, size=(T, B, K, N)).astype(np.float32)
    what = rng.standard_normal((T, B, K, N, N_WHAT)).astype(np.float32)
    lw0 = np.zeros((B, K), np.float32)
    lw = np.zeros((T, B, K), np.float32)
    for b, name in enumerate(names):
        if name == "random":
            lw0[b] = rng.standard_normal(K) * 2
            lw[:, b] = rng.standard_normal((T, K)) * 3
        elif name == "equal":
            lw0[b] = rng.standard_normal() * 5
            lw[:, b] = rng.standard_normal((T, 1))
        elif name == "dominant":
            lw0[b] = -np.inf if b % 2 == 0 else -200.0
            lw0[b, rng.integers(0, K)] = 0.0
        elif name == "spread":
            lw0[b] = -rng.uniform(size=K) * rng.uniform(80, 110)
        elif name == "neg_inf":
            lw0[b] = rng.standard_normal(K)
            dead = rng.uniform(size=K) < 0.4
            dead[rng.integers(0, K)] = False
            lw0[b] = np.where(dead, -np.inf, lw0[b])
            lw[:, b] = rng.standard_normal((T, K))
    lw0[-3, K // 2] = np.nan
    lw0[-2, K - 1] = np.inf
    lw0[-1, :] = -np.inf
    R = B * K
    return (B, where.reshape(T, R, N, 4), pres.reshape(T, R, N), ids.reshape(T, R, N), what.reshape(T, R, N, N_WHAT), lw0.reshape(R),
            lw.reshape(T, R), names)


def _run(lib, h, T, B, K, N, hw, where, pres, ids, what, canvas, lw0, lw, iou_min):
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()
    z = lambda shp, dt=torch.float32: torch.full(shp, -7, dtype=dt, device="cuda")
    i32 = torch.int32
    d = dict(where=dev(where), presence=dev(pres), obj_id=dev(ids), what=dev(what), lw=dev(lw), log_w=dev(lw0))
    o = dict(best_row=z((T, B), i32), weights=z((T, B, K)), ess=z((T, B)), count_prob=z((T, B, N + 1)), expected_count=z((T, B)),
             map_count=z((T, B), i32), presence=z((T, B, N)), obj_id=z((T, B, N)), where=z((T, B, N, 4)), what=z((T, B, N, N_WHAT)),
             box=z((T, B, N, 4)), support=z((T, B, N)), box_mean=z((T, B, N, 4)))
    if canvas is not None:
        d["canvas"] = dev(canvas)
        o["mean_canvas"] = z((T, B) + hw)
    est = _capi.SqairLaneEstimate(iou_min=iou_min, log_w=d["log_w"].data_ptr(), **{k: v.data_ptr() for k, v in o.items()})
    s = torch.cuda.current_stream()
    rc = lib.sqair_lane_estimate_test(h, d["where"].data_ptr(), d["presence"].data_ptr(), d["obj_id"].data_ptr(), d["what"].data_ptr(),
                                      d["canvas"].data_ptr() if canvas is not None else None, d["lw"].data_ptr(), T, B, K,
                                      C.byref(est), C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in o.items()}


_handles = {}


def _handle(wide, N, hw):
    key = (wide, N, hw)
    if key not in _handles:
        _handles[key] = open_handle(_capi.WIDE_LIB_PATH if wide else None, hw, k_particles=2, n_steps_per_image=N, n_what=N_WHAT)
    return _handles[key]


# (K, T, N, wide, hw, iou_min, canvas)
CASES = [(K, T, 4, False, (50, 50), 0.5, K == 5 and T == 3) for K in (1, 2, 5, 64, 65, 256) for T in (1, 3)]
CASES.append((5, 1, 14, True, (50, 50), 0.3, False))        # the wide library: the most slots a handle takes
CASES.append((65, 3, 4, False, (12, 9), 0.7, True))         # H * W no multiple of anything, boxes larger than the frame


@pytest.mark.parametrize("K,T,N,wide,hw,iou_min,with_canvas", CASES,
                         ids=["K{}_T{}_N{}_{}x{}{}".format(c[0], c[1], c[2], c[4][0], c[4][1], "_wide" if c[3] else "") for c in CASES])
def test_estimate_kernel_against_fp64(K, T, N, wide, hw, iou_min, with_canvas):
    lib, h = _handle(wide, N, hw)
    rng = np.random.default_rng(1000 * K + 10 * T + N)
    B, where, pres, ids, what, lw0, lw, names = _lanes(K, T, N, 8 if K > 65 else 12, rng, big_boxes=hw != (50, 50))
    canvas = rng.uniform(size=(T, B * K) + hw).astype(np.float32) if with_canvas else None
    got = _run(lib, h, T, B, K, N, hw, where, pres, ids, what, canvas, lw0, lw, iou_min)
    ref = E.estimate(where, pres, ids, lw, K, hw, iou_min, lw0=lw0, what=what, canvas=canvas)
    assert ref.bad[:, -3:].all() and not ref.bad[:, :-3].any()
    counts = EC.check(got, ref, where, pres, K, hw, iou_min, canvas=canvas, names=names)
    print(K, T, N, hw, counts)
    assert counts["decisions"] > 0 and counts["skipped"] <= 0.01 * counts["decisions"], counts
    assert counts["box_mean_checked"] > 0 and counts["map_checked"] > 0
    assert counts["agreeing"] > 0 and (K == 1 or counts["disagreeing"] > 0), counts


def test_optional_outputs_and_null_log_w():
    """Every pointer but best_row may be NULL, log_w NULL means zeros, and the outputs that are bound do not depend on the others."""
    K, T, N, hw = 5, 2, 4, (50, 50)
    lib, h = _handle(False, N, hw)
    rng = np.random.default_rng(5)
    B, where, pres, ids, what, lw0, lw, _ = _lanes(K, T, N, 1, rng, False)
    full = _run(lib, h, T, B, K, N, hw, where, pres, ids, what, None, np.zeros_like(lw0), lw, 0.5)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).cuda()
    d = [dev(x) for x in (where, pres, ids, lw)]
    best = torch.full((T, B), -7, dtype=torch.int32, device="cuda")
    sup = torch.full((T, B, N), -7.0, device="cuda")
    for kw in (dict(), dict(support=sup.data_ptr())):
        est = _capi.SqairLaneEstimate(iou_min=0.5, log_w=None, best_row=best.data_ptr(), **kw)
        s = torch.cuda.current_stream()
        assert lib.sqair_lane_estimate_test(h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, None, d[3].data_ptr(), T, B, K,
                                            C.byref(est), C.c_void_p(s.cuda_stream)) == 0, lib.sqair_last_error(h)
        torch.cuda.synchronize()
        assert np.array_equal(best.cpu().numpy(), full["best_row"])
    assert np.array_equal(sup.cpu().numpy(), full["support"], equal_nan=True)
