"""No GPU: the float64 reference of trajectory scoring (tests/traj_score_ref.py) held to answers known by hand, and what the GPU test
(tests/test_traj_score_kernel.py) relies on, checked from the reference alone on that test's own inputs (tests/traj_score_cases.py):
the error of an fp32 restatement of pair_iou, centre_err, p_alive and the Brier term against float64 -- the GPU bars are four times
these, taken from the reference and never from the kernel --, the lanes the fragile rule leaves out (none: the seeds are chosen so),
and that every kind of event occurs.  With SQAIR_PARITY_DIR set the figures are written to traj_score_parity.json there (the copy
under profiles/ is such a file, completed by the GPU test); without it nothing is written."""
import json
import os

import numpy as np
import pytest

from tests import traj_score_cases as TC
from tests import traj_score_ref as R

PARITY_DIR_ENV = "SQAIR_PARITY_DIR"
A = (10.0, 10.0, 10.0, 10.0)          # (y, x, h, w)
FAR = (35.0, 35.0, 8.0, 8.0)


def shift(b, dy, dx=0.0):
    return (b[0] + dy, b[1] + dx, b[2], b[3])


def lane(anchor, objects, frames, G, N, valid_mass=None, truth_valid=None, anchor_valid=1, best_row=0):
    """One lane.  anchor {g: box}; objects {j: (box0, id, support)}; frames: a list of ({g: box} present truths, {j: (alive, box_mean)},
    count_prob or None)."""
    F = len(frames)
    tab = dict(best_row=np.array([best_row], np.int32), presence=np.zeros((1, N), np.float32), obj_id=np.zeros((1, N), np.float32),
               support=np.zeros((1, N), np.float32), box0=np.zeros((1, N, 4), np.float32), alive=np.zeros((F, 1, N), np.float32),
               box_mean=np.zeros((F, 1, N, 4), np.float32), count_prob=np.zeros((F, 1, N + 1), np.float32))
    tr = dict(anchor_box=np.zeros((1, G, 4), np.float32), anchor_present=np.zeros((1, G), np.int32),
              anchor_valid=np.array([anchor_valid], np.int32), truth_box=np.zeros((F, 1, G, 4), np.float32),
              truth_present=np.zeros((F, 1, G), np.int32),
              truth_valid=np.ones((F, 1), np.int32) if truth_valid is None else np.array(truth_valid, np.int32).reshape(F, 1))
    for g, bx in anchor.items():
        tr["anchor_box"][0, g], tr["anchor_present"][0, g] = bx, 1
    for j, (bx, i, s) in objects.items():
        tab["box0"][0, j], tab["presence"][0, j], tab["obj_id"][0, j], tab["support"][0, j] = bx, 1.0, i, s
    for f, (truths, objs, cp) in enumerate(frames):
        for g, bx in truths.items():
            tr["truth_box"][f, 0, g], tr["truth_present"][f, 0, g] = bx, 1
        for j, (al, bx) in objs.items():
            tab["alive"][f, 0, j], tab["box_mean"][f, 0, j] = al, bx
        tab["count_prob"][f, 0, len(truths) if cp is None else cp] = 1.0
    if valid_mass is not None:
        tab["valid_mass"] = np.array(valid_mass, np.float32).reshape(F, 1)
    return tab, tr


def counts(s, f=None):
    c = s.counts[:, 0] if f is None else s.counts[f:f + 1, 0]
    return dict(zip(R.COUNTS, c.sum(0).tolist()))


def sums(s, f):
    return dict(zip(R.SUMS, s.sums[f, 0].tolist()))


def test_a_perfect_forecast():
    frames = [({0: shift(A, f + 1)}, {0: (0.5, shift(A, f + 1))}, None) for f in range(3)]
    s = R.score(*lane({0: A}, {0: (A, 1.0, 0.5)}, frames, 1, 2), 0.5)
    assert s.link[0].tolist() == [0] and s.link_iou[0, 0] == 1.0 and s.lane_counts[0].tolist() == [1, 0, 1, 1]
    assert (s.state[:, 0, 0] == 1).all() and (s.pair_iou[:, 0, 0] == 1.0).all() and not s.centre_err.any() and not s.brier.any()
    assert (s.p_alive[:, 0, 0] == 1.0).all()
    c = counts(s)
    assert (c["frames"], c["pairs"], c["hits"], c["lost"], c["gone"], c["count_hit"], c["count_abs_err"]) == (3, 3, 3, 0, 0, 3, 0)
    assert s.sums[:, 0].tolist() == [[1.0, 0.0, 0.0]] * 3
    p = R.pooled(s.counts, s.sums, s.lane_counts)
    assert p["ade"].tolist() == [0, 0, 0] and p["fde"] == 0 and p["mean_iou"].tolist() == [1, 1, 1] and p["link_rate"] == 1.0
    assert p["hit_rate"].tolist() == [1, 1, 1] and p["brier"].tolist() == [0, 0, 0] and p["count_accuracy"].tolist() == [1, 1, 1]


def test_a_box_shifted_by_3_4_is_5_pixels_off():
    s = R.score(*lane({0: A}, {0: (A, 1.0, 1.0)}, [({0: A}, {0: (1.0, shift(A, 3, 4))}, None)], 1, 1), 0.5)
    assert s.centre_err[0, 0, 0] == 5.0 and s.state[0, 0, 0] == 1
    assert abs(s.pair_iou[0, 0, 0] - 42.0 / 158.0) < 1e-15 and counts(s)["hits"] == 0 and counts(s)["pairs"] == 1
    assert sums(s, 0)["centre_err_sum"] == 5.0
    # the centre, not the corner: a box that grows around its centre is not off
    grown = (A[0] - 2, A[1] - 1, A[2] + 4, A[3] + 2)
    s = R.score(*lane({0: A}, {0: (A, 1.0, 1.0)}, [({0: A}, {0: (1.0, grown)}, None)], 1, 1), 0.5)
    assert s.centre_err[0, 0, 0] == 0.0 and 0.5 < s.pair_iou[0, 0, 0] < 1.0 and counts(s)["hits"] == 1


def test_a_truth_that_leaves_gives_the_brier_term_of_the_survival_probability():
    frames = [({0: A}, {0: (1.0, A)}, None), ({0: A}, {0: (1.0, A)}, None), ({}, {0: (0.25, A)}, None)]
    s = R.score(*lane({0: A}, {0: (A, 1.0, 1.0)}, frames, 1, 1), 0.5)
    assert s.state[:, 0, 0].tolist() == [1, 1, 0] and s.p_alive[2, 0, 0] == 0.25 and s.brier[2, 0, 0] == 0.0625
    assert sums(s, 2) == dict(iou_sum=0.0, centre_err_sum=0.0, brier_sum=0.0625) and counts(s, 2)["gone"] == 1
    assert s.pair_iou[2, 0, 0] == 0 and s.centre_err[2, 0, 0] == 0          # a gone truth has no pair: only the Brier term
    assert R.pooled(s.counts, s.sums, s.lane_counts)["brier"].tolist() == [0, 0, 0.0625]
    # alive / support, not alive: half of a support of 0.5 is a survival of 0.5 ... and the truth is there: (0.5 - 1)^2
    s = R.score(*lane({0: A}, {0: (A, 1.0, 0.5)}, [({0: A}, {0: (0.25, A)}, None)], 1, 1), 0.5)
    assert s.p_alive[0, 0, 0] == 0.5 and s.brier[0, 0, 0] == 0.25 and s.state[0, 0, 0] == 1


def test_a_lost_object_never_reads_its_nan_box():
    nan = (float("nan"),) * 4
    frames = [({0: A}, {0: (0.5, A)}, None), ({0: A}, {0: (0.0, nan)}, None)]
    s = R.score(*lane({0: A}, {0: (A, 1.0, 1.0)}, frames, 1, 1), 0.5)
    assert s.state[:, 0, 0].tolist() == [1, 2] and counts(s, 1)["lost"] == 1 and counts(s, 1)["pairs"] == 0
    assert s.brier[1, 0, 0] == 1.0 and s.pair_iou[1, 0, 0] == 0 and s.centre_err[1, 0, 0] == 0 and np.isfinite(s.sums).all()
    p = R.pooled(s.counts, s.sums, s.lane_counts)
    assert p["hit_rate"].tolist() == [1.0, 0.0] and np.isnan(p["ade"][1]) and np.isnan(p["fde"]) and p["brier"].tolist() == [0.25, 1.0]


def test_an_unlinked_truth_counts_for_the_count_alone():
    frames = [({0: A, 1: FAR}, {0: (1.0, A)}, 1)]
    s = R.score(*lane({0: A, 1: FAR}, {0: (A, 1.0, 1.0)}, frames, 2, 2), 0.5)
    assert s.link[0].tolist() == [0, -1] and s.lane_counts[0].tolist() == [1, 0, 2, 1]
    assert s.state[0, 0].tolist() == [1, -1] and s.p_alive[0, 0, 1] == 0 and s.pair_iou[0, 0, 1] == 0
    c = counts(s)
    assert (c["pairs"], c["lost"], c["gone"], c["count_hit"], c["count_abs_err"]) == (1, 0, 0, 0, 1)     # count_map 1, two truths
    assert R.pooled(s.counts, s.sums, s.lane_counts)["link_rate"] == 0.5
    # a truth that is not at the anchor but appears later: never linked, counted among the frame's truths
    frames = [({0: A}, {0: (1.0, A)}, 1), ({0: A, 1: FAR}, {0: (1.0, A)}, 1)]
    s = R.score(*lane({0: A}, {0: (A, 1.0, 1.0)}, frames, 2, 2), 0.5)
    assert s.lane_counts[0].tolist() == [1, 0, 1, 1] and s.counts[:, 0, 5].tolist() == [1, 0] and s.counts[:, 0, 6].tolist() == [0, 1]


def test_keep_against_a_stranger_of_higher_iou():
    word = lambda v: int(np.array(v, np.float32).view(np.int32))
    objects = {0: (A, 7.0, 1.0), 1: (shift(A, 2), 3.0, 1.0)}         # object 0 is the exact copy; object 1 carries the kept id
    tab, tr = lane({0: A}, objects, [({0: A}, {0: (1.0, A), 1: (1.0, shift(A, 2))}, None)], 1, 2)
    assert R.score(tab, tr, 0.5).link[0].tolist() == [0]
    s = R.score(tab, tr, 0.5, keep_id=np.array([[word(3.0)]], np.int32))
    assert s.link[0].tolist() == [1] and abs(s.link_iou[0, 0] - 80.0 / 120.0) < 1e-15 and s.centre_err[0, 0, 0] == 2.0
    assert R.score(tab, tr, 0.7, keep_id=np.array([[word(3.0)]], np.int32)).link[0].tolist() == [0]     # the kept pair must pass iou_min
    assert R.score(tab, tr, 0.5, keep_id=np.array([[word(9.0)]], np.int32)).link[0].tolist() == [0]     # an id nobody carries
    assert R.score(tab, tr, 0.5, keep_id=np.array([[-1]], np.int32)).link[0].tolist() == [0]


def test_the_tie_order():
    # two truths at the same box, two objects at the same box: every IoU is 1 -- (g 0, j 0) first, then (g 1, j 1)
    tab, tr = lane({0: A, 1: A}, {0: (A, 1.0, 1.0), 1: (A, 2.0, 1.0)}, [({0: A, 1: A}, {0: (1.0, A), 1: (1.0, A)}, None)], 2, 2)
    assert R.score(tab, tr, 0.5).link[0].tolist() == [0, 1]
    # holes on both sides: truth slots 1 and 3, object slots 2 and 3
    tab, tr = lane({1: A, 3: A}, {2: (A, 1.0, 1.0), 3: (A, 2.0, 1.0)}, [({1: A, 3: A}, {2: (1.0, A), 3: (1.0, A)}, None)], 4, 4)
    assert R.score(tab, tr, 0.5).link[0].tolist() == [-1, 2, -1, 3]
    # the first argmax of the count
    tab["count_prob"][0, 0] = [0.1, 0.4, 0.4, 0.1, 0.0]
    s = R.score(tab, tr, 0.5)
    assert s.count_map[0, 0] == 1 and counts(s)["count_abs_err"] == 1


def test_an_unreached_or_untruthed_frame_changes_nothing():
    frames = [({0: A}, {0: (1.0, A)}, None)] * 4
    s = R.score(*lane({0: A}, {0: (A, 1.0, 1.0)}, frames, 1, 1, valid_mass=[0.0, 0.5, 1.0, float("nan")], truth_valid=[1, 1, 0, 1]), 0.5)
    assert s.counts[:, 0, 0].tolist() == [0, 1, 0, 0] and s.state[:, 0, 0].tolist() == [-1, 1, -1, -1]
    assert s.count_map[:, 0].tolist() == [-1, 1, -1, -1] and not s.counts[[0, 2, 3]].any() and not s.sums[[0, 2, 3]].any()
    assert s.lane_counts[0].tolist() == [1, 0, 1, 1]                       # the link is made once, whatever the frames


def test_a_lane_without_anchor_is_untouched_and_a_non_finite_lane_counts_one_invalid_call():
    frames = [({0: A}, {0: (1.0, A)}, None)]
    s = R.score(*lane({0: A}, {0: (A, 1.0, 1.0)}, frames, 1, 1, anchor_valid=0), 0.5)
    assert not s.counts.any() and not s.sums.any() and not s.lane_counts.any()
    assert s.link[0, 0] == -1 and s.state[0, 0, 0] == -1 and s.count_map[0, 0] == -1 and s.p_alive[0, 0, 0] == 0
    s = R.score(*lane({0: A}, {0: (A, 1.0, 1.0)}, frames, 1, 1, best_row=-1), 0.5)
    assert not s.counts.any() and not s.sums.any() and s.lane_counts[0].tolist() == [0, 1, 0, 0]
    assert s.link[0, 0] == -1 and s.state[0, 0, 0] == -1 and s.count_map[0, 0] == -1


def test_two_calls_against_one_call_with_doubled_counters():
    c = TC.CASES[1]
    tab, tr, keep = TC.make(c)
    one = R.score(tab, tr, c.iou_min, keep)
    two = R.score(tab, tr, c.iou_min, keep, counts=one.counts, sums=one.sums, lane_counts=one.lane_counts)
    assert np.array_equal(two.counts, 2 * one.counts) and np.array_equal(two.lane_counts, 2 * one.lane_counts)
    assert np.allclose(two.sums, 2 * one.sums, rtol=1e-14, atol=0.0)     # (the terms are added to the cell one by one: float64 rounding)
    for n in R.INT_OUT + R.FLOAT_OUT:
        assert np.array_equal(getattr(one, n), getattr(two, n)), n


def test_pooled_ratios_are_nan_without_a_denominator():
    p = R.pooled(np.zeros((3, 2, 7), np.int64), np.zeros((3, 2, 3)), np.zeros((2, 4), np.int64))
    assert all(np.isnan(v).all() for v in p.values())


# ---- what the GPU test relies on, on its own inputs ---------------------------------------------------------------------------------
def _record(case, **figures):
    where = os.environ.get(PARITY_DIR_ENV)
    if not where:
        return
    path = os.path.join(where, "traj_score_parity.json")
    try:
        os.makedirs(where, exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {
            "note": "per case of tests/traj_score_cases.py.  reference: the worst error of an fp32 NumPy restatement of each float output "
                    "against the float64 reference (tests/test_traj_score_ref.py) -- the GPU test allows four times these -- and the "
                    "lanes the fragile rule leaves out; kernel: the largest error tests/test_traj_score_kernel.py saw on the device "
                    "(sums per term); integer outputs, counts and lane_counts are compared exactly",
            "cases": {}}
        data["cases"].setdefault(case, {})["reference"] = figures
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize("c", TC.CASES, ids=[TC.case_id(c) for c in TC.CASES])
def test_the_gpu_tests_inputs(c):
    tab, tr, keep = TC.make(c)
    assert ("valid_mass" in tab) == c.mass and (keep is not None) == c.keep
    for bx in (tab["box0"], tab["box_mean"], tr["anchor_box"], tr["truth_box"]):      # the quarter-pixel grid
        v = bx[np.isfinite(bx)]
        assert np.array_equal(v * 4, np.round(v * 4))
    s = R.score(tab, tr, c.iou_min, keep)
    err = R.fp32_errors(tab, tr, s)
    bar = R.bars(err)
    print(TC.case_id(c), "fp32 restatement against float64, worst errors:", {n: "{:.3g}".format(e) for n, e in err.items()})
    assert all(0.0 < bar[n] < 1e-5 for n in ("link_iou", "pair_iou", "centre_err", "p_alive", "brier")), bar
    fragile = R.fragile_lanes(tab, tr, s, c.iou_min, max(bar["link_iou"], bar["pair_iou"]))
    tot = dict(zip(R.COUNTS, s.counts.sum((0, 1)).tolist()))
    lanes = dict(zip(R.LANE_COUNTS, s.lane_counts.sum(0).tolist()))
    print(TC.case_id(c), "fragile lanes", int(fragile.sum()), "of", c.B, tot, lanes)
    _record(TC.case_id(c), fp32_error=err, lanes=c.B, left_out=int(fragile.sum()), **tot, **lanes)
    assert fragile.sum() == 0 and fragile.sum() <= TC.FRAGILE_CAP * c.B      # the seeds are chosen so: the cap is never drawn on
    # every kind of event occurs
    assert all(tot[n] > 0 for n in R.COUNTS), tot
    assert lanes["calls"] == c.B - 2 and lanes["calls_invalid"] == 1 and lanes["anchor_truth"] > lanes["linked"] > 0
    nl, il = TC.nan_lane(c), TC.invalid_lane(c)
    assert not s.counts[:, [nl, il]].any() and not s.sums[:, [nl, il]].any() and not s.lane_counts[il].any()
    assert s.lane_counts[nl].tolist() == [0, 1, 0, 0]
    assert (s.state[:, il] == -1).all() and (s.count_map[:, [nl, il]] == -1).all()
    assert tot["hits"] < tot["pairs"] and (s.pair_iou == 1.0).any()
    # a lost object's box is NaN; holes among the lane objects and the truths; lanes with no anchor truth and with all G
    bi = np.arange(c.B)[:, None]
    assert np.isnan(tab["box_mean"][:, bi, np.maximum(s.link, 0)][s.state == 2]).all() and (s.state == 2).any()
    assert ((tab["presence"][:, :-1] == 0) & (tab["presence"][:, 1:] != 0)).any()
    n_anchor = tr["anchor_present"].sum(-1)
    assert (n_anchor == 0).any() and (n_anchor == c.G).any()
    assert ((tr["truth_present"] != 0) & (tr["anchor_present"] == 0)[None]).any()          # born after the anchor: never linked
    assert np.isfinite(s.sums).all()
    if c.mass:
        skipped = (tab["valid_mass"] == 0) & (tr["truth_valid"] != 0) & R.lane_on(tab, tr)[None]
        assert skipped.any() and not s.counts[skipped].any() and (s.count_map[skipped] == -1).all()
    if c.keep and c.G > 1:      # the keep changes some links: a kept pair is not always the best one
        assert (R.score(tab, tr, c.iou_min, None).link != s.link).any()
    if c.F > 256:   # the second trip of the frame stride is scored
        assert s.counts[256:, :, 0].any() and s.counts[256:, :, 1].any()
