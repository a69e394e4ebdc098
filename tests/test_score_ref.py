"""No GPU: the float64 reference of stream scoring (tests/score_ref.py) on answers known by hand, and what the GPU test relies on,
checked on the very inputs it uses (tests/score_cases.py): the error of an fp32 restatement of sq_box_iou against float64 (printed;
four times it is the GPU test's tolerance for ``match_iou`` and must stay below 1e-5), the cap of 1 % on the lanes left out as
fragile, and that every counter is exercised."""
import numpy as np
import pytest

from tests import score_cases as SC
from tests import score_ref as R

f32 = np.float32


def _lane(frames, G, N, valid=None, map_count=None):
    """One lane from ``frames`` = [(truths {g: box}, objects {j: (box, id)})]: the arguments of R.score."""
    T = len(frames)
    tb, tp = np.zeros((T, 1, G, 4), f32), np.zeros((T, 1, G), np.int32)
    bx, pr, oid = np.zeros((T, 1, N, 4), f32), np.zeros((T, 1, N), f32), np.zeros((T, 1, N), f32)
    for t, (truths, objs) in enumerate(frames):
        for g, b in truths.items():
            tb[t, 0, g], tp[t, 0, g] = b, 1
        for j, (b, i) in objs.items():
            bx[t, 0, j], pr[t, 0, j], oid[t, 0, j] = b, 1.0, i
    mc = pr.sum(-1).astype(np.int32) if map_count is None else np.asarray(map_count, np.int32).reshape(T, 1)
    va = np.ones((T, 1), np.int32) if valid is None else np.asarray(valid, np.int32).reshape(T, 1)
    return bx, pr, oid, mc, tb, tp, va


def _counts(s):
    return dict(zip(R.COUNTS, s.counts[0].tolist()))


A, Bx, Cx = (10, 10, 10, 10), (30, 30, 10, 10), (10, 30, 8, 8)
shift = lambda b, dy: (b[0] + dy, b[1], b[2], b[3])


def test_a_perfect_tracker_has_mota_1_and_motp_1():
    frames = [({0: shift(A, t), 2: shift(Bx, t)}, {1: (shift(A, t), 5.0), 0: (shift(Bx, t), 7.0)}) for t in range(4)]   # (holes on both sides)
    s = R.score(*_lane(frames, 3, 3), 0.5)
    assert _counts(s) == dict(frames=4, frames_invalid=0, truth=8, tp=8, fn=0, fp=0, idsw=0, count_hit=4, count_abs_err=0)
    assert R.pooled(s.counts, s.iou_sum) == dict(mota=1.0, motp=1.0, count_accuracy=1.0)
    assert (s.truth_match[:, 0] == [1, -1, 0]).all() and (s.match_iou[:, 0] == [1, 0, 1]).all()
    assert s.last_id[0].tolist() == [R.words(f32(5.0)).item(), -1, R.words(f32(7.0)).item()]


def test_two_objects_swapping_ids_count_two_switches():
    frames = [({0: A, 1: Bx}, {0: (A, 1.0), 1: (Bx, 2.0)}), ({0: A, 1: Bx}, {0: (A, 2.0), 1: (Bx, 1.0)}), ({0: A, 1: Bx}, {0: (A, 2.0), 1: (Bx, 1.0)})]
    s = R.score(*_lane(frames, 2, 2), 0.5)
    c = _counts(s)
    assert c["idsw"] == 2 and c["tp"] == 6 and c["fn"] == c["fp"] == 0 and s.idsw[:, 0].tolist() == [0, 2, 0]
    assert R.pooled(s.counts, s.iou_sum)["mota"] == 1.0 - 2.0 / 6.0


def test_a_dropped_detection_keeps_the_memory_and_a_new_id_counts_once():
    frames = [({0: A}, {0: (A, 3.0)}), ({0: A}, {}), ({0: A}, {0: (A, 4.0)}), ({0: A}, {0: (A, 4.0)})]
    s = R.score(*_lane(frames, 1, 2), 0.5)
    assert s.idsw[:, 0].tolist() == [0, 0, 1, 0] and s.fn[:, 0].tolist() == [0, 1, 0, 0]
    c = _counts(s)
    assert (c["idsw"], c["tp"], c["fn"], c["fp"], c["count_hit"], c["count_abs_err"]) == (1, 3, 1, 0, 3, 1)
    # ... and in two passes, the state handed on: the same
    a = R.score(*[x[:2] for x in _lane(frames, 1, 2)], 0.5)
    assert a.last_id[0, 0] == R.words(f32(3.0)).item()
    b = R.score(*[x[2:] for x in _lane(frames, 1, 2)], 0.5, counts=a.counts, iou_sum=a.iou_sum, last_id=a.last_id)
    assert (b.counts == s.counts).all() and (b.iou_sum == s.iou_sum).all() and (b.last_id == s.last_id).all()


def test_keep_beats_a_stranger_of_higher_iou():
    near, exact = shift(A, 2), A    # IoU 2/3 and 1 with truth A
    frames = [({0: A}, {0: (A, 3.0)}), ({0: A}, {0: (exact, 9.0), 1: (near, 3.0)})]
    s = R.score(*_lane(frames, 1, 2), 0.5)
    assert s.truth_match[1, 0, 0] == 1 and s.idsw[1, 0] == 0 and s.fp[1, 0] == 1 and abs(s.match_iou[1, 0, 0] - 2.0 / 3.0) < 1e-12
    # below iou_min the known id is not kept: the stranger is taken and the switch counted
    s = R.score(*_lane(frames, 1, 2), 0.7)
    assert s.truth_match[1, 0, 0] == 0 and s.idsw[1, 0] == 1
    # an absent slot carrying the known id is no candidate
    bx, pr, oid, mc, tb, tp, va = _lane(frames, 1, 2)
    pr[1, 0, 1] = 0.0
    s = R.score(bx, pr, oid, mc, tb, tp, va, 0.5)
    assert s.truth_match[1, 0, 0] == 0 and s.idsw[1, 0] == 1 and s.fp[1, 0] == 0


def test_greedy_takes_the_maximum_and_breaks_ties_by_g_then_j():
    # truths 0 and 1 the same box, objects 0 and 1 the same box: four candidates of IoU exactly 1 -> (0, 0), then (1, 1)
    s = R.score(*_lane([({0: A, 1: A}, {0: (A, 1.0), 1: (A, 2.0)})], 2, 2), 0.5)
    assert s.truth_match[0, 0].tolist() == [0, 1]
    # the maximum first, whatever its indices
    T0, T1 = (10, 10, 10, 10), (10, 14, 10, 10)
    O0, O1 = (10, 14, 10, 10), (10, 6, 10, 10)      # O0 = T1; IoU(T0, O0) = 0.43, IoU(T0, O1) = 0.43, IoU(T1, O1) = 1/9
    s = R.score(*_lane([({0: T0, 1: T1}, {0: (O0, 1.0), 1: (O1, 2.0)})], 2, 2), 0.3)
    assert s.truth_match[0, 0].tolist() == [1, 0] and s.tp[0, 0] == 2     # the maximum first: (1, 0) at IoU 1, then (0, 1)
    s = R.score(*_lane([({0: T0, 1: T1}, {0: (O0, 1.0)})], 2, 2), 0.3)
    assert s.truth_match[0, 0].tolist() == [-1, 0] and (s.tp[0, 0], s.fn[0, 0]) == (1, 1)
    # a NaN never wins
    nan = (float("nan"), 10, 10, 10)
    s = R.score(*_lane([({0: A}, {0: (nan, 1.0), 1: (shift(A, 3), 2.0)})], 1, 2), 0.5)
    assert s.truth_match[0, 0, 0] == 1 and s.fp[0, 0] == 1


def test_an_invalid_frame_changes_nothing():
    frames = [({0: A}, {0: (A, 3.0)}), ({0: A}, {0: (A, 8.0), 1: (Bx, 1.0)}), ({0: A}, {0: (A, 3.0)})]
    s = R.score(*_lane(frames, 1, 2, valid=[1, 0, 1]), 0.5)
    c = _counts(s)
    assert (c["frames"], c["tp"], c["fp"], c["idsw"], c["truth"]) == (2, 2, 0, 0, 2)
    assert s.tp[:, 0].tolist() == [1, -1, 1] and s.truth_match[1, 0, 0] == -1 and s.match_iou[1, 0, 0] == 0


def test_a_non_finite_lane_counts_one_invalid_frame_and_nothing_else():
    frames = [({0: A}, {0: (A, 3.0)}), ({0: A}, {}), ({0: A}, {0: (A, 4.0)})]
    s = R.score(*_lane(frames, 1, 2, map_count=[1, -1, 1]), 0.5)
    c = _counts(s)
    assert (c["frames"], c["frames_invalid"], c["truth"], c["fn"], c["idsw"]) == (2, 1, 2, 0, 1)
    assert s.fn[:, 0].tolist() == [0, -1, 0]
    s = R.score(*_lane(frames, 1, 2, map_count=[1, -1, 1], valid=[1, 0, 1]), 0.5)      # without truth it is not even counted
    assert _counts(s)["frames_invalid"] == 0


def test_pooled_ratios_are_nan_without_a_denominator():
    p = R.pooled(np.zeros((2, 9), np.int64), np.zeros(2))
    assert all(np.isnan(v) for v in p.values())


# ---- what the GPU test relies on, on its own inputs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("c", SC.CASES, ids=[SC.case_id(c) for c in SC.CASES])
def test_the_gpu_tests_inputs(c):
    x = SC.make(c)
    err = R.iou32_error(x["truth_box"], x["box"])
    print(SC.case_id(c), "fp32 restatement of sq_box_iou against float64: worst error {:.3g}; the GPU test allows {:.3g}".format(err, 4 * err))
    assert 0.0 < 4 * err < 1e-5
    s = R.score(iou_min=c.iou_min, **x)
    first = R.fragile_from(s.iou, x["presence"], x["map_count"], x["truth_present"], x["truth_valid"], c.iou_min)
    out = int((first < SC.T).sum())
    tot = dict(zip(R.COUNTS, s.counts.sum(0).tolist()))
    print(SC.case_id(c), "fragile lanes", out, "of", SC.B, tot)
    assert out <= SC.FRAGILE_CAP * SC.B
    assert all(tot[n] > 0 for n in R.COUNTS), tot
    assert tot["frames_invalid"] == SC.T - SC.NAN_FROM and not s.counts[SC.INVALID_LANE].any()
    assert tot["truth"] == tot["tp"] + tot["fn"] and tot["idsw"] >= 20 and min(tot["tp"], tot["fn"], tot["fp"]) >= 100
    # lanes with no truth and lanes with all G; holes among the lane objects; exact copies
    n_truth = x["truth_present"].sum(-1)
    assert (n_truth.max(0) == 0).any() and (n_truth.min(0) == c.G).any()
    assert ((x["presence"][:, :, :-1] == 0) & (x["presence"][:, :, 1:] != 0)).any()
    assert (s.match_iou == 1.0).any() and ((s.match_iou > 0) & (s.match_iou < 1)).any()
