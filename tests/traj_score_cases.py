"""The inputs of tests/test_traj_score_kernel.py (GPU) and of the checks tests/test_traj_score_ref.py makes on the very same arrays
(CPU): lane tables and truth trajectories built directly, no stream.  Frames of 50 x 50 pixels, every box on a quarter-pixel grid.
Cases: (G, N) = (4, 4), (1, 4) and, on the wide library, (16, 14); iou_min 0.5 and 0.3; 210 lanes of F = 5 frames, and 8 lanes of
F = 300 (the frame stride's second trip); with and without valid_mass (zeros in it); with and without keep_id.

Anchor truth: boxes of 8-28 px at -5..45 px; a slot is present with probability 0.7, every 7th lane has none, every 5th all G; in a
fifth of the lanes truth 1 is truth 0 moved by 2-3 px, so that two truths compete for the same lane objects.  The truth then moves
with a velocity; some truths end at a later frame, some absent slots are born at one (present, never linked).  Lane objects: per
anchor-present truth a detection = its box plus a jitter of up to 0, 0.5, 2 or 6 px per lane (every 11th lane: exact copies), kept with
probability 0.85, a spurious object with probability 0.3, at most N; present-first in the even lanes, shuffled with holes in the odd
ones; absent slots are zeros.  support in [0.3, 1]; alive = support times a survival that falls over the frames in steps of 1/4,
reaching 0 for some objects -- box_mean is NaN from there on; else box_mean = the truth's box plus a jitter that grows with the frame.
count_prob: random masses with the odd exact tie.  keep_id: the linked object's own id word, a stranger's, or -1.  A tenth of the
(frame, lane)s have no truth.  One lane is non-finite (best_row -1, NaN table), one has an invalid anchor."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "G N iou_min wide B F mass keep seed")
CASES = [Case(4, 4, 0.5, False, 210, 5, False, False, 1451), Case(4, 4, 0.3, False, 210, 5, True, True, 4432),
         Case(1, 4, 0.5, False, 210, 5, True, False, 151), Case(1, 4, 0.3, False, 210, 5, False, True, 131),
         Case(16, 14, 0.5, True, 210, 5, False, True, 1651), Case(16, 14, 0.3, True, 210, 5, True, False, 4631),
         Case(4, 4, 0.5, False, 8, 300, True, False, 12451), Case(16, 14, 0.3, True, 8, 300, False, True, 87631)]
HW, K = (50, 50), 2
FRAGILE_CAP = 0.01      # of the lanes; the seeds are chosen so that the reference leaves out none (tests/test_traj_score_ref.py)


def case_id(c):
    return "G{}_N{}_iou{:g}_B{}_F{}{}{}{}".format(c.G, c.N, c.iou_min, c.B, c.F, "_mass" if c.mass else "", "_keep" if c.keep else "",
                                                  "_wide" if c.wide else "")


def nan_lane(c):
    return 7 if c.B > 8 else 3


def invalid_lane(c):
    return 9 if c.B > 8 else 5


def _grid(x):
    return np.round(np.asarray(x, np.float64) * 4.0) / 4.0


@functools.lru_cache(maxsize=None)
def make(c):
    """(table, truth, keep_id or None): {name: array} in the C ABI's names; made once, never written to."""
    rng = np.random.default_rng(c.seed)
    G, N, B, F = c.G, c.N, c.B, c.F
    f32 = np.float32
    lanes = np.arange(B)
    # ---- the anchor truth and its trajectories
    a_box = np.concatenate([_grid(rng.uniform(-5, 45, (B, G, 2))), _grid(rng.uniform(8, 28, (B, G, 2)))], -1)
    if G >= 2:
        twin = lanes % 5 == 2
        a_box[twin, 1] = a_box[twin, 0] + np.concatenate([_grid(rng.uniform(2, 3, (int(twin.sum()), 2))), np.zeros((int(twin.sum()), 2))], -1)
    a_pres = rng.uniform(size=(B, G)) < 0.7
    a_pres[lanes % 7 == 3] = False
    a_pres[lanes % 5 == 1] = True
    if G >= 2:
        a_pres[twin, :2] = True
    vel = _grid(rng.uniform(-2.5, 2.5, (B, G, 2)))
    t = np.arange(1, F + 1)[:, None, None, None]
    truth_box = np.concatenate([a_box[None, :, :, :2] + vel[None] * np.minimum(t, 12), np.broadcast_to(a_box[None, :, :, 2:], (F, B, G, 2))], -1)
    end = np.where(rng.uniform(size=(B, G)) < 0.3, rng.integers(1, F + 1, (B, G)), F)
    born = np.where(~a_pres & (rng.uniform(size=(B, G)) < 0.3), rng.integers(0, F - 1, (B, G)), F)
    ff = np.arange(F)[:, None, None]
    truth_present = np.where(a_pres[None], ff < end[None], ff >= born[None]).astype(np.int32)
    truth_valid = (rng.uniform(size=(F, B)) >= 0.1).astype(np.int32)
    anchor_valid = np.ones(B, np.int32)
    anchor_valid[invalid_lane(c)] = 0
    # ---- the lane table
    jitter = np.array([0.0, 0.5, 2.0, 6.0])[rng.integers(0, 4, B)]
    jitter[lanes % 11 == 0] = 0.0
    presence, obj_id, support = np.zeros((B, N), f32), np.zeros((B, N), f32), np.zeros((B, N), f32)
    box0 = np.zeros((B, N, 4), f32)
    alive, box_mean = np.zeros((F, B, N), f32), np.zeros((F, B, N, 4), f32)
    keep_id = -np.ones((B, G), np.int32)
    word = lambda v: int(np.array(v, f32).view(np.int32))
    for b in range(B):
        hyp = int(rng.integers(0, 5))
        dets = []                      # (box0, id, truth slot or -1)
        for g in range(G):
            if a_pres[b, g] and rng.uniform() < 0.85:
                noisy = a_box[b, g] + _grid(jitter[b] * rng.uniform(-1, 1, 4))
                noisy[2:] = np.maximum(noisy[2:], 1.0)
                dets.append((noisy, float(1 + g + 100 * hyp), g))
        if rng.uniform() < 0.3:
            dets.append((np.concatenate([_grid(rng.uniform(-5, 45, 2)), _grid(rng.uniform(8, 28, 2))]), float(90 + 100 * hyp), -1))
        dets = dets[:N]
        slots = rng.permutation(N)[:len(dets)] if b % 2 else np.arange(len(dets))
        for s, (bx, i, g) in zip(slots, dets):
            presence[b, s], obj_id[b, s], box0[b, s], support[b, s] = 1.0, i, bx, rng.uniform(0.3, 1.0)
            surv = 1.0
            walk = _grid(rng.uniform(-2.5, 2.5, 2))
            for f in range(F):
                if rng.uniform() < min(0.15, 1.0 / F):
                    surv = max(surv - 0.25 * int(rng.integers(1, 3)), 0.0)
                alive[f, b, s] = f32(support[b, s]) * f32(surv)
                if surv == 0.0:
                    box_mean[f, b, s] = np.nan
                elif g >= 0:
                    box_mean[f, b, s] = truth_box[f, b, g] + _grid(min(0.25 * jitter[b] * (f + 1), 8.0) * rng.uniform(-1, 1, 4))
                    box_mean[f, b, s, 2:] = np.maximum(box_mean[f, b, s, 2:], 1.0)
                else:
                    box_mean[f, b, s] = np.concatenate([bx[:2] + walk * min(f + 1, 12), bx[2:]])
        ids = [word(i) for _, i, _ in dets]
        for g in range(G):             # the identity memory: the own detection's id, a stranger's, or none
            r = rng.uniform()
            own = [word(i) for _, i, gg in dets if gg == g]
            if r < 0.5 and own:
                keep_id[b, g] = own[0]
            elif r < 0.7 and ids:
                keep_id[b, g] = ids[int(rng.integers(0, len(ids)))]
    count_prob = rng.uniform(size=(F, B, N + 1)) ** 3
    tie = rng.uniform(size=(F, B)) < 0.1
    count_prob[tie, 1] = count_prob[tie].max(-1)     # (an exact tie with a later or an earlier maximum: the first one wins)
    count_prob = (count_prob / count_prob.sum(-1, keepdims=True)).astype(f32)
    count_prob[tie, 1] = count_prob[tie].max(-1)
    valid_mass = np.where(rng.uniform(size=(F, B)) < 0.15, 0.0, rng.uniform(0.05, 1.0, (F, B))).astype(f32)
    best_row = (lanes * K + rng.integers(0, K, B)).astype(np.int32)
    nl = nan_lane(c)
    best_row[nl] = -1
    presence[nl], obj_id[nl], box0[nl], support[nl] = 0.0, 0.0, 0.0, np.nan
    alive[:, nl], box_mean[:, nl], count_prob[:, nl], valid_mass[:, nl] = np.nan, np.nan, np.nan, np.nan
    table = dict(best_row=best_row, presence=presence, obj_id=obj_id, support=support, box0=box0, alive=alive, box_mean=box_mean,
                 count_prob=count_prob)
    if c.mass:
        table["valid_mass"] = valid_mass
    truth = dict(anchor_box=a_box.astype(f32), anchor_present=a_pres.astype(np.int32), anchor_valid=anchor_valid,
                 truth_box=truth_box.astype(f32), truth_present=truth_present, truth_valid=truth_valid)
    keep = keep_id if c.keep else None
    for a in list(table.values()) + list(truth.values()) + ([keep] if c.keep else []):
        a.setflags(write=False)
    return table, truth, keep
