"""The inputs of tests/test_score_kernel.py (GPU) and of the checks tests/test_score_ref.py makes on the very same arrays (CPU): 210
lanes of T = 6 frames of 50 x 50 pixels per case, (G, N) = (4, 4), (1, 4) and, on the wide library, (16, 14), iou_min 0.5 and 0.3.

Truth: boxes of 8-28 px at -5..45 px moving with a velocity, born in frames 0-2, some dying in the last two; absent truths keep their
moving box (presence alone must decide); every 7th lane has no truth, every 5th all G for all frames.  Lane answer: per present
truth a detection = its box plus sigma N(0, 1), sigma in {0.3, 2, 6} px per lane (every 11th lane: exact copies), kept with
probability 0.85, a spurious box with probability 0.2, at most N in all.  Ids: 1 + g + 100 * (the lane's hypothesis), the hypothesis
redrawn with probability 0.1 per frame; in a quarter of the lanes the ids of truths 0 and 1 are swapped from frame 3 on.  Slots:
present-first in the even lanes, shuffled with holes in the odd ones; absent slots are zeros.  map_count: the number of detections,
off by one in a fifth of the frames.  Lane 7 is non-finite from frame 2 on (map_count -1, no objects), lane 9 has no valid frame,
and a tenth of the other (frame, lane)s are invalid."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "G N iou_min wide seed")
CASES = [Case(G, N, iou, wide, 100 * G + int(10 * iou)) for G, N, wide in ((4, 4, False), (1, 4, False), (16, 14, True)) for iou in (0.5, 0.3)]
B, T, HW = 210, 6, (50, 50)
NAN_LANE, NAN_FROM, INVALID_LANE = 7, 2, 9
FRAGILE_CAP = 0.01      # of the lanes


def case_id(c):
    return "G{}_N{}_iou{:g}{}".format(c.G, c.N, c.iou_min, "_wide" if c.wide else "")


@functools.lru_cache(maxsize=None)
def make(c):
    """{name: array} for the case; made once, never written to."""
    rng = np.random.default_rng(c.seed)
    G, N = c.G, c.N
    f32 = np.float32
    # ---- truth
    size = rng.uniform(8, 28, (B, G, 2))
    pos0 = rng.uniform(-5, 45, (B, G, 2))
    vel = rng.uniform(-2.5, 2.5, (B, G, 2))
    t = np.arange(T)[:, None, None, None]
    truth_box = np.concatenate([pos0[None] + vel[None] * t, np.broadcast_to(size[None], (T, B, G, 2))], -1).astype(f32)   # (y, x, h, w)
    birth = rng.integers(0, 3, (B, G))
    death = np.where(rng.uniform(size=(B, G)) < 0.3, rng.integers(T - 2, T, (B, G)), T)
    alive = rng.uniform(size=(B, G)) < 0.7
    lanes = np.arange(B)
    alive[lanes % 7 == 3] = False
    full = lanes % 5 == 1
    alive[full], birth[full], death[full] = True, 0, T
    tt = np.arange(T)[:, None, None]
    truth_present = (alive[None] & (tt >= birth[None]) & (tt < death[None])).astype(np.int32)
    truth_valid = (rng.uniform(size=(T, B)) >= 0.1).astype(np.int32)
    truth_valid[:, INVALID_LANE] = 0
    truth_valid[:, NAN_LANE] = 1
    # ---- the lane answer
    sigma = np.array([0.3, 2.0, 6.0])[rng.integers(0, 3, B)]
    sigma[lanes % 11 == 0] = 0.0
    box = np.zeros((T, B, N, 4), f32)
    presence = np.zeros((T, B, N), f32)
    obj_id = np.zeros((T, B, N), f32)
    map_count = np.zeros((T, B), np.int32)
    swap = (lanes % 4 == 2) & (G >= 2)
    for b in range(B):
        hyp = int(rng.integers(0, 5))
        for f in range(T):
            if rng.uniform() < 0.1:
                hyp = int(rng.integers(5, 50))
            dets = []
            for g in range(G):
                if truth_present[f, b, g] and rng.uniform() < 0.85:
                    gid = (1 - g if g < 2 else g) if (swap[b] and f >= 3) else g
                    noisy = truth_box[f, b, g].astype(np.float64) + sigma[b] * rng.standard_normal(4)
                    noisy[2:] = np.maximum(noisy[2:], 1.0)
                    dets.append((truth_box[f, b, g] if sigma[b] == 0.0 else noisy.astype(f32), f32(1 + gid + 100 * hyp)))
            if rng.uniform() < 0.2:
                dets.append((np.concatenate([rng.uniform(-5, 45, 2), rng.uniform(8, 28, 2)]).astype(f32), f32(90 + 100 * hyp)))
            dets = dets[:N]
            slots = rng.permutation(N)[:len(dets)] if b % 2 else np.arange(len(dets))
            for s, (bx, i) in zip(slots, dets):
                box[f, b, s], presence[f, b, s], obj_id[f, b, s] = bx, 1.0, i
            off = int(rng.integers(-1, 2)) if rng.uniform() < 0.2 else 0
            map_count[f, b] = min(max(len(dets) + off, 0), N)
    box[NAN_FROM:, NAN_LANE], presence[NAN_FROM:, NAN_LANE], obj_id[NAN_FROM:, NAN_LANE] = 0.0, 0.0, 0.0
    map_count[NAN_FROM:, NAN_LANE] = -1
    out = dict(box=box, presence=presence, obj_id=obj_id, map_count=map_count, truth_box=truth_box, truth_present=truth_present,
               truth_valid=truth_valid)
    for a in out.values():
        a.setflags(write=False)
    return out
