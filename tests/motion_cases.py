"""The inputs of tests/test_motion_kernel.py (and of the reference-only checks of tests/test_motion_ref.py): the scenes of
tests/identity_cases.py for B = 200 lanes over T = 12 frames with a PER-OBJECT CONSTANT VELOCITY added to the random walk.

A lane holds N + 2 objects of which at most N are visible at a time.  Every object has a box on a random walk (about 0.5 px a frame)
plus its own velocity -- half of the objects are slow (up to 1 px a frame per axis), the others fast (up to 8 px a frame per axis, well
beyond what the IoU gate follows from the last box) -- reflected at the edges of the field, a ``what`` vector of its own and an
obj_id that is a per-lane counter value.  Per frame and visible object: with probability 0.15 its obj_id changes to a fresh value (a
best-row switch); with probability 0.2 it drops out for 1..5 frames (max_age is 3: drop-outs of 4 and 5 frames end the track) and
KEEPS MOVING while it is hidden -- a moving drop-out --; one return in five has jumped well outside any gate instead.  Some lanes keep
an object in the slot of its index (holes), the others list the visible objects present-first.  Lane NAN_LANE is non-finite (best_row
= -1, its other inputs garbage that must not be read) from frame NAN_FROM on; lane EMPTY_LANE never shows an object.

The shapes are the smallest at which the kernel can go wrong: (M, N, n_what) = (8, 4, 50); (4, 4, 50), a full table in which every birth
evicts; (1, 1, 1); (16, 14, 128) on the wide library, where 224 threads fill the tables; one case without trk_what, where d2 ranks the
re-identification; one with the position link keep + optimal."""
import collections
import functools

import numpy as np

T, B = 12, 200
HW = (50, 50)
MAX_AGE = 3
IOU_MIN = 0.3
REID_DIST = 4.0          # (with motion on: only the on/off switch of re-identification)
Q, R_MEAS, V0_VAR, GATE = 0.25, 1.0, 16.0, 3.0
V_MAX = 8.0
NAN_LANE, NAN_FROM, EMPTY_LANE = 7, 3, 11
FRAGILE_CAP = 0.02      # the share of lanes that may be left out as fragile
LO, HI = -10.0, 60.0    # the field the boxes' corners stay in

Case = collections.namedtuple("Case", "M N nw wide appearance optimal seed")
CASES = (Case(8, 4, 50, False, True, False, 1),
         Case(4, 4, 50, False, True, False, 2),
         Case(1, 1, 1, False, True, False, 3),
         Case(16, 14, 128, True, True, False, 4),
         Case(8, 4, 50, False, False, False, 5),
         Case(8, 4, 50, False, True, True, 6))


def case_id(c):
    return "M{}_N{}_nw{}{}{}{}".format(c.M, c.N, c.nw, "_wide" if c.wide else "", "" if c.appearance else "_nowhat",
                                       "_optimal" if c.optimal else "")


def make(c):
    """{box [T, B, N, 4], presence, obj_id [T, B, N], what [T, B, N, nw] float32, best_row [T, B] int32} of case ``c``."""
    rng = np.random.default_rng(2000 + c.seed)
    N, nw = c.N, c.nw
    n_obj = N + 2
    box = np.zeros((T, B, N, 4), np.float32)
    presence = np.zeros((T, B, N), np.float32)
    obj_id = np.zeros((T, B, N), np.float32)
    what = np.zeros((T, B, N, nw), np.float32)
    best_row = np.zeros((T, B), np.int32)
    for b in range(B):
        pos = np.concatenate([rng.uniform(0, 40, (n_obj, 2)), rng.uniform(8, 16, (n_obj, 2))], 1)     # (y, x, h, w)
        fast = rng.uniform(size=n_obj) < 0.5
        vel = rng.uniform(-1, 1, (n_obj, 2)) * np.where(fast, V_MAX, 1.0)[:, None]
        look = rng.standard_normal((n_obj, nw))
        ids = np.arange(n_obj, dtype=np.float64)
        next_id = float(n_obj)
        hidden = np.where(rng.uniform(size=n_obj) < 0.5, 0, rng.integers(1, 4, n_obj))      # frames until the object may show
        unseen = np.zeros(n_obj, np.int64)                                                    # frames since it was last shown
        shown_before = np.zeros(n_obj, bool)
        holes = b % 3 == 0 and n_obj > N
        for t in range(T):
            best_row[t, b] = b * 3 + int(rng.integers(0, 3))
            pos[:, :2] += vel + rng.normal(0, 0.5, (n_obj, 2))        # every object moves on, seen or not
            for a in range(2):                                        # reflected at the edges
                out = (pos[:, a] < LO) | (pos[:, a] + pos[:, 2 + a] > HI)
                vel[out, a] = -vel[out, a]
                pos[:, a] = np.clip(pos[:, a], LO, HI - pos[:, 2 + a])
            visible = []
            for k in range(n_obj):
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
                    elif shown_before[k] and rng.uniform() < 0.2:   # a return that has jumped: outside every gate
                        a = rng.uniform(0, 2 * np.pi)
                        pos[k, :2] += rng.uniform(25, 35) * np.array([np.sin(a), np.cos(a)])
                        pos[k, :2] = np.clip(pos[k, :2], LO, HI - pos[k, 2:])
                    if len(visible) < N:
                        visible.append(k)
                        continue
                unseen[k] += 1
            for n, k in enumerate(visible):
                j = k % N if holes else n
                while presence[t, b, j] != 0:                    # (holes: the object's own slot, or the next free one)
                    j = (j + 1) % N
                pos[k, 2:] = np.clip(pos[k, 2:] + rng.normal(0, 0.3, 2), 6, 20)
                box[t, b, j] = pos[k]
                presence[t, b, j] = 1.0
                obj_id[t, b, j] = ids[k]
                what[t, b, j] = look[k] + 0.05 * rng.standard_normal(nw)
                shown_before[k], unseen[k] = True, 0
    presence[:, EMPTY_LANE] = 0
    best_row[NAN_FROM:, NAN_LANE] = -1
    garbage = rng.standard_normal((T - NAN_FROM, N, 4)).astype(np.float32)
    box[NAN_FROM:, NAN_LANE] = garbage * 30
    presence[NAN_FROM:, NAN_LANE] = 1.0
    obj_id[NAN_FROM:, NAN_LANE] = 77.0
    what[NAN_FROM:, NAN_LANE] = np.nan
    return dict(box=box, presence=presence, obj_id=obj_id, what=what, best_row=best_row)


SCALARS = (Q, R_MEAS, V0_VAR, GATE)


@functools.lru_cache(maxsize=None)
def reference(i):
    """(inputs, the float64 reference, the fragility band, fragile_from [B]) of case i: made once per process, never written to."""
    from tests import motion_ref as MR
    c = CASES[i]
    x = make(c)
    ref = MR.identity(iou_min=IOU_MIN, reid_dist=REID_DIST, reid_what=float("inf"), M=c.M, max_age=MAX_AGE, motion=SCALARS,
                      appearance=c.appearance, optimal=c.optimal, **x)
    tol = MR.measured_tol(ref.err)
    return x, ref, tol, MR.fragile_from(ref.margins, tol)


# ---- the two hand-made scenarios (one 10 x 10 object per lane, N = 1): they fail without the feature ---------------------------------
def scenario(centres, seen):
    """{box [T, 1, 1, 4], presence, obj_id [T, 1, 1], what [T, 1, 1, 1], best_row [T, 1]} of one 10 x 10 object whose CENTRE is
    centres[t] = (cy, cx) in the frames where seen[t], absent elsewhere; obj_id 5 throughout."""
    centres = np.asarray(centres, np.float64)
    n = len(centres)
    box = np.zeros((n, 1, 1, 4), np.float32)
    box[:, 0, 0, :2], box[:, 0, 0, 2:] = centres - 5.0, 10.0
    presence = np.asarray(seen, np.float32).reshape(n, 1, 1)
    box *= presence[..., None]
    return dict(box=box, presence=presence, obj_id=5.0 * presence, what=np.zeros((n, 1, 1, 1), np.float32),
                best_row=np.zeros((n, 1), np.int32))


def fast_mover(step=(8.0, 0.0), frames=6):
    """Six frames of an object moving ``step`` px a frame from centre (10, 10)."""
    return scenario([(10.0 + step[0] * t, 10.0 + step[1] * t) for t in range(frames)], [1] * frames)


DROP_SEEN = (1, 1, 1, 1, 1, 0, 0, 0, 0, 1, 1)


def moving_dropout(sigma=0.0, seed=0):
    """Eleven frames of an object moving 3 px a frame along y from centre (10, 20), seen in frames 0-4 and 9-10; ``sigma``: the
    standard deviation of the measurement noise added to the centre (fixed seed).  Returns (inputs, the true centres)."""
    true = np.array([(10.0 + 3.0 * t, 20.0) for t in range(len(DROP_SEEN))])
    noise = np.random.default_rng(seed).normal(0, 1, true.shape) * sigma
    return scenario(true + noise, DROP_SEEN), true
