"""The inputs of tests/test_hota_kernel.py and tests/test_hota_solve_kernel.py (GPU) and of the checks tests/test_hota_ref.py makes on
the very same arrays (CPU): 24 lanes of T = 40 frames per case, (G, N, P, L) = (4, 4, 32, 64), (1, 4, 8, 16) and, on the wide library,
(16, 14, 64, 32).

Every box coordinate is a multiple of a quarter pixel (as in tests/traj_score_cases.py): the fp32 products and sums of sq_box_iou are
then exact and only its one division rounds.  Truths move on straight lines, are born and die; a lane answer detects a present truth
with probability 0.85 at an offset of 0, 1/4 .. 2 or up to 6 pixels per coordinate and adds a false positive to every fifth frame.
By lane: b % 5 == 1 is CROWDED (every truth alive, all starting within twelve pixels of each other); in b % 4 == 2 the ids of truths 0
and 1 SWITCH for the middle third of the clip and RETURN; in b % 3 == 0 every object draws a new id in every frame, so that the clip
sees more ids than P columns; b % 13 == 5 gives its first present object a negative id, b % 17 == 4 repeats the first object's id on
the second.  Lane 7 is non-finite (map_count -1) from frame 2 on, lane 9 has no truthed frame, every other lane loses a tenth of its
frames' truth; with T = 40 every lane of the cases with L = 16 and L = 32 that is scored throughout has more scored frames than L."""
import collections
import ctypes as C
import functools

import numpy as np
import torch

from sqair_amd import _capi
from tests import hota_ref as R
from tests import score_ref as SR
from tests.abi_host import LANE_LIBS, kept_handle

Case = collections.namedtuple("Case", "G N P L wide seed")
CASES = [Case(4, 4, 32, 64, False, 4432), Case(1, 4, 8, 16, False, 1408), Case(16, 14, 64, 32, True, 1614)]
B, T, HW = 24, 40, (50, 50)
NAN_LANE, NAN_FROM, INVALID_LANE = 7, 2, 9
INPUTS = ("box", "presence", "ids", "map_count", "truth_box", "truth_present", "truth_valid")


def case_id(c):
    return "G{}_N{}_P{}_L{}{}".format(c.G, c.N, c.P, c.L, "_wide" if c.wide else "")


def _quarter(v):
    return np.round(np.asarray(v, np.float64) * 4.0) / 4.0


@functools.lru_cache(maxsize=None)
def make(c):
    """{name: array} for the case; made once, never written to."""
    rng = np.random.default_rng(c.seed)
    G, N, f32 = c.G, c.N, np.float32
    lanes = np.arange(B)
    crowded = lanes % 5 == 1
    size = _quarter(rng.uniform(8, 20, (B, G, 2)))
    pos0 = _quarter(np.where(crowded[:, None, None], rng.uniform(10, 22, (B, G, 2)), rng.uniform(-5, 40, (B, G, 2))))
    vel = _quarter(np.where(crowded[:, None, None], rng.uniform(-0.25, 0.25, (B, G, 2)), rng.uniform(-0.75, 0.75, (B, G, 2))))
    t = np.arange(T)[:, None, None, None]
    truth_box = np.concatenate([pos0[None] + vel[None] * t, np.broadcast_to(size[None], (T, B, G, 2))], -1).astype(f32)
    birth = rng.integers(0, 6, (B, G))
    death = np.where(rng.uniform(size=(B, G)) < 0.3, rng.integers(T - 12, T, (B, G)), T)
    alive = rng.uniform(size=(B, G)) < 0.8
    alive[crowded], birth[crowded], death[crowded] = True, 0, T
    tt = np.arange(T)[:, None, None]
    truth_present = (alive[None] & (tt >= birth[None]) & (tt < death[None])).astype(np.int32)
    truth_valid = (rng.uniform(size=(T, B)) >= 0.1).astype(np.int32)
    truth_valid[:, INVALID_LANE] = 0
    truth_valid[:, NAN_LANE] = 1
    steps = [np.zeros(1), np.arange(-8, 9) / 4.0, np.arange(-24, 25) / 4.0]
    noise = rng.integers(0, 3, B)
    box, presence = np.zeros((T, B, N, 4), f32), np.zeros((T, B, N), f32)
    obj_id, map_count = np.zeros((T, B, N), f32), np.zeros((T, B), np.int32)
    for b in range(B):
        for f in range(T):
            dets = []
            for g in range(G):
                if truth_present[f, b, g] and rng.uniform() < 0.85:
                    gid = (1 - g if g < 2 else g) if (b % 4 == 2 and G >= 2 and T // 3 <= f < 2 * T // 3) else g
                    bx = truth_box[f, b, g].astype(np.float64) + rng.choice(steps[noise[b]], 4)
                    bx[2:] = np.maximum(bx[2:], 1.0)
                    dets.append((bx.astype(f32), f32(1 + gid)))
            if rng.uniform() < 0.2:
                dets.append((_quarter(np.concatenate([rng.uniform(-5, 40, 2), rng.uniform(8, 20, 2)])).astype(f32), f32(90)))
            dets = dets[:N]
            slots = rng.permutation(N)[:len(dets)] if b % 2 else np.arange(len(dets))
            for s, (bx, i) in zip(slots, dets):
                box[f, b, s], presence[f, b, s], obj_id[f, b, s] = bx, 1.0, i
            here = np.flatnonzero(presence[f, b] != 0)
            if b % 3 == 0:
                for j in here:
                    obj_id[f, b, j] = f32(1 + j + 100 * int(rng.integers(0, 400)))
            if b % 13 == 5 and here.size:
                obj_id[f, b, here[0]] = f32(-3.0)
            if b % 17 == 4 and here.size >= 2:
                obj_id[f, b, here[1]] = obj_id[f, b, here[0]]
            map_count[f, b] = len(dets)
    box[NAN_FROM:, NAN_LANE], presence[NAN_FROM:, NAN_LANE], obj_id[NAN_FROM:, NAN_LANE] = 0.0, 0.0, 0.0
    map_count[NAN_FROM:, NAN_LANE] = -1
    out = dict(box=box, presence=presence, ids=SR.words(obj_id).copy(), map_count=map_count, truth_box=truth_box,
               truth_present=truth_present, truth_valid=truth_valid)
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the solve on caller logs (GPU)
RTOL = 1e-12


def record(section, case, **figures):
    """One case's figures into hota_parity.json under SQAIR_PARITY_DIR."""
    from tests.kernel_unit import merge_parity

    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data[section][case] = figures
    merge_parity("hota_parity.json", R.fresh_parity, update)


def handle(lib_name, N=4):
    return kept_handle(("hota", lib_name, N), LANE_LIBS[lib_name], HW, k_particles=2, n_steps_per_image=N, n_what=6)


def to_device(log, G, P):
    d = {n: torch.from_numpy(np.array(v)).cuda() for n, v in log.items()}
    d["work"] = torch.full((log["col_id"].shape[0], G, P, _capi.HOTA_BINS), 12345, dtype=torch.int32, device="cuda")   # any content
    return d


def struct(d, P, L):
    return _capi.SqairLaneHota(P=P, L=L, **{n: d[n].data_ptr() for n in _capi.HOTA_LOG + _capi.HOTA_TOTALS})


def run_solve(lib_name, d, G, N, P, L, close=None, want=("open_i", "open_f", "open_c", "match"), stream=None):
    """One launch on the device log ``d`` (updated in place); returns {name: array} of the outputs asked for."""
    lib, h = handle(lib_name)
    n = d["col_id"].shape[0]
    shapes = _capi.hota_solve_shapes(n, G, L)
    out = {k: torch.full(shapes[k], -7, dtype=getattr(torch, _capi.field_dtype("sqair_lane_hota_solve", k)), device="cuda") for k in want}
    mask = None if close is None else torch.from_numpy(np.asarray(close, np.int32)).cuda()
    ptr = lambda k: out[k].data_ptr() if k in out else None
    rc = lib.sqair_lane_hota_solve(h, C.byref(struct(d, P, L)), G, N, n, None if mask is None else mask.data_ptr(), ptr("open_i"),
                                   ptr("open_f"), ptr("open_c"), ptr("match"), C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def judged(log, got, close=None):
    """Judges the device's ``match`` of every record in use on the reference's tables, imposes it, and returns the reference's
    (log after, open_i, open_f, open_c) with the number of records judged and of those whose matching is not SciPy's own."""
    _, _, _, _, own, tables = R.solve(log)
    B, L, G = got["match"].shape
    n = differ = 0
    for b in range(B):
        F = int(log["frames"][b])
        assert (got["match"][b, F:] == -7).all(), (b, F, got["match"][b, F:])      # the records not in use: nothing is written
        for r in range(F):
            R.judge(tables[b][r], got["match"][b, r])
            n += 1
            differ += not np.array_equal(got["match"][b, r], own[b, r])
    after, oi, of, oc, _, _ = R.solve(log, close=close, match=got["match"])
    return after, oi, of, oc, n, differ


def close_enough(a, b):
    return np.allclose(a, b, rtol=RTOL, atol=0.0)
