"""The inputs of tests/test_identity_kernel.py (and of the reference-only checks of tests/test_identity_ref.py): what the estimate
would hand k_lane_identity for B = 200 lanes over T = 8 frames, made from a small scene per lane.

A lane holds N + 2 objects of which at most N are visible at a time.  Every object has a box on a random walk (about 1 px a frame), a
``what`` vector of its own (plus a little noise per frame) and an obj_id that is a per-lane counter value.  Per frame and visible object:
with probability 0.15 its obj_id changes to a fresh value -- a best-row switch -- and in half of those frames the box keeps the very
words of the frame before; with probability 0.2 it drops out for 1..5 frames (max_age is 3: drop-outs of 4 and 5 frames end the track).
An object that returns has walked on (inside the IoU gate or just outside it), or has jumped beyond the IoU gate but inside
reid_dist * (age + 1), or has jumped outside that gate too.  Some lanes keep an object in the slot of its index (holes), the others list
the visible objects present-first.  Lane NAN_LANE is non-finite (best_row = -1, its other inputs garbage that must not be read) from
frame NAN_FROM on; lane EMPTY_LANE never shows an object.

The shapes are the smallest at which the kernel can go wrong: (M, N, n_what) = (8, 4, 50); (4, 4, 50), a full table in which every birth
evicts; (1, 1, 1); (16, 14, 128) on the wide library, where 224 threads fill the tables; one case without trk_what; one with a finite
reid_what; one with re-identification off."""
import collections

import numpy as np

T, B = 8, 200
HW = (50, 50)
MAX_AGE = 3
IOU_MIN = 0.3
REID_DIST = 4.0
NAN_LANE, NAN_FROM, EMPTY_LANE = 7, 3, 11
FRAGILE_CAP = 0.02      # the share of lanes that may be left out as fragile

Case = collections.namedtuple("Case", "M N nw wide appearance reid_dist reid_what seed")
CASES = (Case(8, 4, 50, False, True, REID_DIST, float("inf"), 1),
         Case(8, 4, 50, False, True, REID_DIST, 0.5, 2),
         Case(4, 4, 50, False, True, REID_DIST, float("inf"), 3),
         Case(1, 1, 1, False, True, REID_DIST, float("inf"), 4),
         Case(16, 14, 128, True, True, REID_DIST, float("inf"), 5),
         Case(8, 4, 50, False, False, REID_DIST, float("inf"), 6),
         Case(8, 4, 50, False, True, 0.0, float("inf"), 7))


def case_id(c):
    return "M{}_N{}_nw{}{}{}{}{}".format(c.M, c.N, c.nw, "_wide" if c.wide else "", "" if c.appearance else "_nowhat",
                                         "" if c.reid_dist > 0 else "_noreid", "" if np.isinf(c.reid_what) else "_what{}".format(c.reid_what))


def make(c):
    """{box [T, B, N, 4], presence, obj_id [T, B, N], what [T, B, N, nw] float32, best_row [T, B] int32} of case ``c``."""
    rng = np.random.default_rng(1000 + c.seed)
    N, nw = c.N, c.nw
    n_obj = N + 2
    box = np.zeros((T, B, N, 4), np.float32)
    presence = np.zeros((T, B, N), np.float32)
    obj_id = np.zeros((T, B, N), np.float32)
    what = np.zeros((T, B, N, nw), np.float32)
    best_row = np.zeros((T, B), np.int32)
    for b in range(B):
        pos = np.concatenate([rng.uniform(0, 36, (n_obj, 2)), rng.uniform(8, 16, (n_obj, 2))], 1)     # (y, x, h, w)
        look = rng.standard_normal((n_obj, nw))
        ids = np.arange(n_obj, dtype=np.float64)
        next_id = float(n_obj)
        hidden = np.where(rng.uniform(size=n_obj) < 0.5, 0, rng.integers(1, 4, n_obj))      # frames until the object may show
        unseen = np.zeros(n_obj, np.int64)                                                    # frames since it was last shown
        shown_before = np.zeros(n_obj, bool)
        holes = b % 3 == 0 and n_obj > N
        for t in range(T):
            best_row[t, b] = b * 3 + int(rng.integers(0, 3))
            visible = []
            for k in range(n_obj):
                frozen = False
                if hidden[k] > 0:
                    hidden[k] -= 1
                else:
                    if shown_before[k] and unseen[k] == 0:      # shown in the frame before
                        u = rng.uniform()
                        if u < 0.2:
                            hidden[k] = int(rng.integers(1, 6)) - 1
                            unseen[k] += 1
                            continue
                        if u < 0.35:
                            ids[k], next_id = next_id, next_id + 1.0
                            frozen = rng.uniform() < 0.5
                    elif shown_before[k]:                        # a return after unseen[k] frames
                        r = REID_DIST * (unseen[k] + 1)
                        u, a = rng.uniform(), rng.uniform(0, 2 * np.pi)
                        if u < 0.35:       # beyond the IoU gate, inside the re-identification gate
                            pos[k, :2] += rng.uniform(0.55, 0.9) * r * np.array([np.sin(a), np.cos(a)])
                        elif u < 0.6:      # outside both
                            pos[k, :2] += rng.uniform(1.3, 2.0) * r * np.array([np.sin(a), np.cos(a)])
                    if len(visible) < N:
                        visible.append((k, frozen))
                        continue
                unseen[k] += 1
            for n, (k, frozen) in enumerate(visible):
                j = k % N if holes else n
                while presence[t, b, j] != 0:                    # (holes: the object's own slot, or the next free one)
                    j = (j + 1) % N
                if not frozen:
                    pos[k] += np.concatenate([rng.normal(0, 1.0, 2), rng.normal(0, 0.3, 2)])
                    pos[k, 2:] = np.clip(pos[k, 2:], 6, 20)
                pos[k, :2] = np.clip(pos[k, :2], -10, 50)        # (near the frame: the fp32 error of dc2 grows with the coordinates)
                box[t, b, j] = pos[k]
                presence[t, b, j] = 1.0
                obj_id[t, b, j] = ids[k]
                what[t, b, j] = look[k] + 0.05 * rng.standard_normal(nw)
                shown_before[k], unseen[k] = True, 0
            for k in range(n_obj):                               # the hidden walk on
                if not any(k == v for v, _ in visible):
                    pos[k, :2] += rng.normal(0, 1.0, 2)
    presence[:, EMPTY_LANE] = 0
    best_row[NAN_FROM:, NAN_LANE] = -1
    garbage = rng.standard_normal((T - NAN_FROM, N, 4)).astype(np.float32)
    box[NAN_FROM:, NAN_LANE] = garbage * 30
    presence[NAN_FROM:, NAN_LANE] = 1.0
    obj_id[NAN_FROM:, NAN_LANE] = 77.0
    what[NAN_FROM:, NAN_LANE] = np.nan
    return dict(box=box, presence=presence, obj_id=obj_id, what=what, best_row=best_row)
