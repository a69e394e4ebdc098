"""The inputs of tests/test_match_kernel.py (GPU) and of the checks tests/test_match_ref.py makes on the very same arrays (CPU): crowded
lanes in the shape of tests/score_cases.py -- 200 lanes of T = 8 frames of 50 x 50 pixels per case, (G, N) = (1, 1), (2, 2), (4, 4),
(3, 4) and, on the wide library, (16, 14), iou_min 0.5 and 0.3.

Truth: the truths of a lane are a CROWD -- boxes whose corners lie within a pixel or so of the lane's own centre (30-38 px boxes;
G = 16: 14-22 px boxes spread over 9 px), each truth's size within 2 px of the lane's, so that they overlap each other heavily,
drifting together with a small velocity of their own; three in four born in frame 0, the others in frame 1, some dying in the last
two; absent truths keep their moving box; every 25th lane has no truth.  Lane answer: per present truth a detection = its box plus
sigma N(0, 1), sigma in {2, 3, 4, 6} px per lane, kept with probability 0.97, then a spurious box inside the crowd with probability
0.3, at most N in all.  Ids: 1 + g + 100 * (the lane's hypothesis), the hypothesis redrawn with probability 0.9 per frame (the keep
step then has nothing to keep and the rest decides; one frame in ten, and the hand cases, exercise the keep); in a quarter of the
lanes the ids of truths 0 and 1 are swapped from frame 4 on.  Slots: present-first in the even lanes, shuffled with holes in the odd
ones; absent slots are zeros.  map_count: the number of detections.  Lane 7 is non-finite from frame 3 on (map_count -1, no
objects), lane 9 has no valid frame, and a tenth of the other (frame, lane)s are invalid.  ``identity_inputs`` and ``traj_inputs``
hand the same lane answer to the identity and to the trajectory link."""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "G N iou_min wide seed")
SHAPES = ((1, 1, False), (2, 2, False), (4, 4, False), (3, 4, False), (16, 14, True))
# (the seed of the one case whose first seed left more than FRAGILE_CAP of the lanes out is moved on: tests/test_match_ref.py)
SEED_SHIFT = {(16, 14, 0.3): 700}
CASES = [Case(G, N, iou, wide, 1000 * G + 10 * N + int(10 * iou) + SEED_SHIFT.get((G, N, iou), 0)) for G, N, wide in SHAPES
         for iou in (0.5, 0.3)]
B, T, HW, NW = 200, 8, (50, 50), 6
NAN_LANE, NAN_FROM, INVALID_LANE = 7, 3, 9
FRAGILE_CAP = 0.01      # of the lanes (the score's)
IDENTITY_M = {(1, 1): (1,), (4, 4): (4, 8), (16, 14): (16,)}     # (G, N) of the case -> the M its lane answer is linked with
TRAJ_F = 3
# (tuned from the reference alone until greedy and optimal differ in a tenth of the scored frames of every case with G, N >= 2:
#  tests/test_match_ref.py)
SPREAD_SMALL, SIZE_SMALL, REDRAW, P_ALIVE, P_DETECT = 1.0, (30, 38), 0.9, 0.97, 0.97


def case_id(c):
    return "G{}_N{}_iou{:g}{}".format(c.G, c.N, c.iou_min, "_wide" if c.wide else "")


@functools.lru_cache(maxsize=None)
def make(c):
    """{name: array} for the case; made once, never written to."""
    rng = np.random.default_rng(c.seed)
    G, N = c.G, c.N
    f32 = np.float32
    # ---- truth: a crowd per lane
    centre = rng.uniform(8, 28, (B, 1, 2))
    spread = SPREAD_SMALL if G <= 4 else 9.0
    size = (rng.uniform(*SIZE_SMALL, (B, 1, 2)) if G <= 4 else rng.uniform(14, 22, (B, 1, 2))) + rng.uniform(-2, 2, (B, G, 2))
    pos0 = centre + rng.normal(0.0, spread, (B, G, 2))
    vel = rng.uniform(-1.0, 1.0, (B, 1, 2)) + rng.uniform(-0.7, 0.7, (B, G, 2))
    t = np.arange(T)[:, None, None, None]
    truth_box = np.concatenate([pos0[None] + vel[None] * t, np.broadcast_to(size[None], (T, B, G, 2))], -1).astype(f32)   # (y, x, h, w)
    birth = (rng.uniform(size=(B, G)) < 0.25).astype(np.int64)
    death = np.where(rng.uniform(size=(B, G)) < 0.15, rng.integers(T - 2, T, (B, G)), T)
    alive = rng.uniform(size=(B, G)) < P_ALIVE
    lanes = np.arange(B)
    alive[lanes % 25 == 4] = False
    tt = np.arange(T)[:, None, None]
    truth_present = (alive[None] & (tt >= birth[None]) & (tt < death[None])).astype(np.int32)
    truth_valid = (rng.uniform(size=(T, B)) >= 0.1).astype(np.int32)
    truth_valid[:, INVALID_LANE] = 0
    truth_valid[:, NAN_LANE] = 1
    # ---- the lane answer
    sigma = np.array([2.0, 3.0, 4.0, 6.0])[rng.integers(0, 4, B)]
    box = np.zeros((T, B, N, 4), f32)
    presence = np.zeros((T, B, N), f32)
    obj_id = np.zeros((T, B, N), f32)
    map_count = np.zeros((T, B), np.int32)
    swap = (lanes % 4 == 2) & (G >= 2)
    for b in range(B):
        hyp = int(rng.integers(0, 5))
        for f in range(T):
            if rng.uniform() < REDRAW:
                hyp = int(rng.integers(5, 50))
            dets = []
            for g in range(G):
                if truth_present[f, b, g] and rng.uniform() < P_DETECT:
                    gid = (1 - g if g < 2 else g) if (swap[b] and f >= 4) else g
                    noisy = truth_box[f, b, g].astype(np.float64) + sigma[b] * rng.standard_normal(4)
                    noisy[2:] = np.maximum(noisy[2:], 1.0)
                    dets.append((noisy.astype(f32), f32(1 + gid + 100 * hyp)))
            if rng.uniform() < 0.3:
                spur = np.concatenate([centre[b, 0] + vel[b, 0] * f + rng.normal(0.0, 4.0, 2), rng.uniform(14, 24, 2)])
                dets.append((spur.astype(f32), f32(90 + 100 * hyp)))
            dets = dets[:N]
            slots = rng.permutation(N)[:len(dets)] if b % 2 else np.arange(len(dets))
            for s, (bx, i) in zip(slots, dets):
                box[f, b, s], presence[f, b, s], obj_id[f, b, s] = bx, 1.0, i
            map_count[f, b] = len(dets)
    box[NAN_FROM:, NAN_LANE], presence[NAN_FROM:, NAN_LANE], obj_id[NAN_FROM:, NAN_LANE] = 0.0, 0.0, 0.0
    map_count[NAN_FROM:, NAN_LANE] = -1
    out = dict(box=box, presence=presence, obj_id=obj_id, map_count=map_count, truth_box=truth_box, truth_present=truth_present,
               truth_valid=truth_valid)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def identity_inputs(c):
    """What k_lane_identity is handed for the case's lane answer: box, presence, obj_id, what [T, B, N, NW], best_row [T, B] (-1 where
    the lane is non-finite)."""
    x = make(c)
    rng = np.random.default_rng(c.seed + 1)
    what = rng.standard_normal((T, B, c.N, NW)).astype(np.float32)
    best_row = np.where(x["map_count"] == -1, -1, 0).astype(np.int32)
    out = dict(box=x["box"], presence=x["presence"], obj_id=x["obj_id"], what=what, best_row=best_row)
    for a in out.values():
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def traj_inputs(c):
    """(table, truth, keep_id) for sqair_lane_traj_score from the case: the anchor is frame 0 -- its truth against its lane answer, the
    crowded link --, the table's TRAJ_F frames are frames 1.. of the case (box_mean = the lane answer's box, alive in (0, 1] or 0,
    support 1); keep_id [B, G]: the id word of a random present object of frame 0, or -1."""
    x = make(c)
    rng = np.random.default_rng(c.seed + 2)
    F, N, G = TRAJ_F, c.N, c.G
    alive = np.where(rng.uniform(size=(F, B, N)) < 0.85, rng.uniform(0.1, 1.0, (F, B, N)), 0.0).astype(np.float32)
    prob = rng.uniform(0.0, 1.0, (F, B, N + 1)).astype(np.float32)
    tab = dict(best_row=np.where(x["map_count"][0] == -1, -1, 0).astype(np.int32), presence=np.array(x["presence"][0]),
               obj_id=np.array(x["obj_id"][0]), support=np.ones((B, N), np.float32), box0=np.array(x["box"][0]), alive=alive,
               box_mean=np.array(x["box"][1:1 + F]), count_prob=(prob / prob.sum(-1, keepdims=True)).astype(np.float32))
    tab["best_row"][NAN_LANE] = -1
    tr = dict(anchor_box=np.array(x["truth_box"][0]), anchor_present=np.array(x["truth_present"][0]),
              anchor_valid=np.array(x["truth_valid"][0]), truth_box=np.array(x["truth_box"][1:1 + F]),
              truth_present=np.array(x["truth_present"][1:1 + F]), truth_valid=np.array(x["truth_valid"][1:1 + F]))
    words = np.ascontiguousarray(tab["obj_id"]).view(np.int32)
    pick = rng.integers(0, N, (B, G))
    keep = np.where((rng.uniform(size=(B, G)) < 0.4) & (np.take_along_axis(tab["presence"], pick, 1) != 0),
                    np.take_along_axis(words, pick, 1), -1).astype(np.int32)
    for a in list(tab.values()) + list(tr.values()) + [keep]:
        a.setflags(write=False)
    return tab, tr, keep


# ---- answers known by hand ---------------------------------------------------------------------------------------------------------
HAND_G, HAND_N, HAND_IOU = 6, 4, 0.5
HAND = ("cardinality", "sum", "keep_wins", "nothing_eligible", "more_truths_than_objects", "fewer_truths_than_objects", "nan_box")


def _row(x, w=20.0):
    """A box of height 20 at y = 0: only x and the width differ (the IoU is then a matter of intervals)."""
    return (0.0, float(x), 20.0, float(w))


@functools.lru_cache(maxsize=None)
def hand():
    """One frame of len(HAND) lanes, G = 6 truth slots and N = 4 object slots, iou_min 0.5, absent slots zeros: (inputs as ``make``'s,
    last_id [B, G] to start from, expect = the optimal mode's truth_match [1, B, G] and tp, fn, fp [1, B], greedy = the greedy mode's
    tp, fn, fp [1, B]).  Every optimum here is unique.  The IoUs, all of boxes of equal y and h:
      cardinality  widths 20 at x = 4 (o1), 10 (t0), 15 (o0), 21 (t1): IoU(t0, o0) = 15/25, IoU(t0, o1) = IoU(t1, o0) = 14/26,
                   IoU(t1, o1) = 3/37.  Greedy takes (t0, o0) and t1 is left with nothing; the optimum is t0-o1, t1-o0.
      sum          t0 at 0, t1 at 3, o0 at 1, o1 at -2: 19/21, 18/22, 18/22, 15/25.  Greedy 19/21 + 15/25 = 1.505; the optimum takes
                   the two 18/22 = 1.636.
      keep_wins    the boxes of `cardinality`, and t0 remembers the id of o0: the kept pair (t0, o0) costs the second pair.
      nothing_eligible            two truths, three objects, every IoU below 0.5.
      more_truths_than_objects    five truths in slots 0, 1, 3, 4, 5 (a hole at 2), two objects in slots 1 and 3.
      fewer_truths_than_objects   two truths in slots 1 and 4, three objects in slots 0, 2, 3; greedy finds one pair of the two.
      nan_box      the boxes of `cardinality` with a NaN for the width of o0: its area, the union and so the IoU are not positive
                   numbers -- a NaN never passes --, t0 takes o1, o0 is a false positive."""
    Bh, G, N = len(HAND), HAND_G, HAND_N
    tb, tp_ = np.zeros((1, Bh, G, 4), np.float32), np.zeros((1, Bh, G), np.int32)
    ob, op, oi = np.zeros((1, Bh, N, 4), np.float32), np.zeros((1, Bh, N), np.float32), np.zeros((1, Bh, N), np.float32)
    last = -np.ones((Bh, G), np.int32)
    match = -np.ones((1, Bh, G), np.int32)

    def put(lane, truths, objects):
        for g, bx in truths.items():
            tb[0, lane, g], tp_[0, lane, g] = bx, 1
        for j, (bx, i) in objects.items():
            ob[0, lane, j], op[0, lane, j], oi[0, lane, j] = bx, 1.0, i
    chain_t, chain_o = {0: _row(10), 1: _row(21)}, {0: (_row(15), 5.0), 1: (_row(4), 6.0)}
    put(0, chain_t, chain_o)
    match[0, 0, :2] = (1, 0)
    put(1, {0: _row(0), 1: _row(3)}, {0: (_row(1), 5.0), 1: (_row(-2), 6.0)})
    match[0, 1, :2] = (1, 0)
    put(2, chain_t, chain_o)
    last[2, 0] = np.float32(5.0).view(np.int32)
    match[0, 2, :2] = (0, -1)
    put(3, {0: _row(0), 2: _row(30)}, {0: (_row(14), 5.0), 1: (_row(45), 6.0), 3: (_row(-15), 7.0)})
    put(4, {0: _row(0), 1: _row(6), 3: _row(12), 4: _row(40), 5: _row(18)}, {1: (_row(8), 5.0), 3: (_row(14), 6.0)})
    match[0, 4, 1], match[0, 4, 3] = 1, 3          # IoU(t1, o1) = 18/22, IoU(t3, o3) = 18/22: 1.636; t1-o3, t3-o1 give 12/28 + 16/24
    put(5, {1: _row(0), 4: _row(5)}, {0: (_row(9), 5.0), 2: (_row(3), 6.0), 3: (_row(-9), 7.0)})
    match[0, 5, 1], match[0, 5, 4] = 2, 0          # t1-o2 17/23, t4-o0 16/24; greedy takes t4-o2 = 18/22 and t1 is left with 11/29 twice
    put(6, chain_t, chain_o)
    ob[0, 6, 0, 3] = np.nan
    match[0, 6, :2] = (1, -1)
    x = dict(box=ob, presence=op, obj_id=oi, map_count=op.sum(-1).astype(np.int32), truth_box=tb, truth_present=tp_,
             truth_valid=np.ones((1, Bh), np.int32))
    n_t, n_o, tp = tp_.sum(-1), op.sum(-1).astype(np.int64), (match >= 0).sum(-1)
    expect = dict(truth_match=match, tp=tp, fn=n_t - tp, fp=n_o - tp)
    gtp = np.array([[1, 2, 1, 0, 2, 1, 1]])
    greedy = dict(tp=gtp, fn=n_t - gtp, fp=n_o - gtp)
    for a in list(x.values()) + [last] + list(expect.values()) + list(greedy.values()):
        a.setflags(write=False)
    return x, last, expect, greedy
