"""No GPU: the float64 reference of the lane forecast (tests/forecast_lane_ref.py) against known answers, the properties the header
states, and the condition on the GPU test's inputs: for its exact seeds, association decisions within 1e-5 of the threshold (or of a
tie) are at most 1 % of all decisions -- the cap tests/test_estimate_kernel.py uses.  A condition the generator meets, not a tolerance."""
import numpy as np
import pytest

from tests import estimate_ref as E
from tests import forecast_lane_ref as FL

HW = (50, 50)


def _one(where_start, where_roll, pres_roll, ids_start, ids_roll, K, S, lw=None, iou_min=0.5):
    ws = np.asarray(where_start, np.float32)
    R, N = ws.shape[:2]
    ps = np.ones((R, N), np.float32)
    return FL.lane_forecast(ws, ps, np.asarray(ids_start, np.float32), np.asarray(where_roll, np.float32),
                            np.asarray(pres_roll, np.float32), np.asarray(ids_roll, np.float32), lw, K, S, HW, iou_min)


def test_single_rollout_is_its_own_answer():
    """K = 1, S = 1: box_mean = the rollout's box, box_std = 0, alive in {0, 1}; the object dies at frame 2 and stays dead; its id
    moves from slot 1 to slot 0 at frame 1 (compaction)."""
    rng = np.random.default_rng(0)
    ws = rng.standard_normal((1, 2, 4))
    wr = rng.standard_normal((3, 1, 2, 4))
    ids_s = [[3.0, 7.0]]
    pres = [[[1, 1]], [[1, 0]], [[0, 0]]]
    ids_r = [[[3.0, 7.0]], [[7.0, -1.0]], [[-1.0, -1.0]]]
    o = _one(ws, wr, pres, ids_s, ids_r, 1, 1)
    assert o.best_row[0] == 0 and (o.support == 1).all() and (o.weights == 1).all()
    assert np.array_equal(o.alive[:, 0], [[1, 1], [0, 1], [0, 0]])
    bx = E.boxes(wr.astype(np.float32), HW)
    assert np.array_equal(o.box_mean[0, 0], bx[0, 0]) and np.array_equal(o.box_mean[1, 0, 1], bx[1, 0, 0])   # id 7 now in slot 0
    assert (o.box_std[0, 0] == 0).all() and (o.box_std[1, 0, 1] == 0).all()
    assert np.isnan(o.box_mean[1, 0, 0]).all() and np.isnan(o.box_std[2, 0]).all()
    assert np.array_equal(o.count_prob[:, 0], [[0, 0, 1], [0, 1, 0], [1, 0, 0]])


def test_two_rollouts_by_hand():
    """K = 1, S = 2, one object: mean and std of two equally weighted boxes; K = 2, S = 1 with weights 3 : 1."""
    ws = np.zeros((1, 1, 4))
    wr = np.zeros((1, 2, 1, 4))
    wr[0, 1, 0, 2] = 0.5                                           # the second rollout moved in x
    o = _one(ws, wr, np.ones((1, 2, 1)), [[4.0]], np.full((1, 2, 1), 4.0), 1, 2)
    bx = E.boxes(wr.astype(np.float32), HW)[0, :, 0]
    assert o.alive[0, 0, 0] == 1.0
    assert np.allclose(o.box_mean[0, 0, 0], (bx[0] + bx[1]) / 2, rtol=0, atol=1e-12)
    assert np.allclose(o.box_std[0, 0, 0], np.abs(bx[0] - bx[1]) / 2, rtol=0, atol=1e-12)
    assert o.box_std[0, 0, 0, 1] > 1.0 and o.box_std[0, 0, 0, 0] == 0.0
    ws2 = np.zeros((2, 1, 4))
    lw = np.log(np.array([3.0, 1.0], np.float32))
    o = _one(ws2, wr, np.ones((1, 2, 1)), [[4.0], [9.0]], np.array([[[4.0], [9.0]]]), 2, 1, lw=lw)
    w = o.weights[0]
    assert np.allclose(w, [0.75, 0.25], atol=1e-7)
    mean = w[0] * bx[0] + w[1] * bx[1]
    assert np.allclose(o.box_mean[0, 0, 0], mean, atol=1e-12)
    assert np.allclose(o.box_std[0, 0, 0], np.sqrt(w[0] * (bx[0] - mean) ** 2 + w[1] * (bx[1] - mean) ** 2), atol=1e-12)
    # the second particle's rollout loses the id: only the first one is left, alive = its weight
    o = _one(ws2, wr, np.ones((1, 2, 1)), [[4.0], [9.0]], np.array([[[4.0], [8.0]]]), 2, 1, lw=lw)
    assert np.isclose(o.alive[0, 0, 0], w[0]) and np.allclose(o.box_mean[0, 0, 0], bx[0]) and (o.box_std[0, 0, 0] < 1e-12).all()
    assert o.support[0, 0] == 1.0


@pytest.mark.parametrize("case", FL.CASES, ids=[FL.case_id(c) for c in FL.CASES])
def test_gpu_cases_properties_and_threshold_cap(case):
    K, S, F, N, wide, hw, iou_min = case
    g = FL.case_inputs(case)
    ref = FL.lane_forecast(g.start_where, g.start_presence, g.start_obj_id, g.where, g.presence, g.obj_id, g.log_w, K, S, hw, iou_min)
    B = g.B
    fin = ~ref.bad
    assert ref.bad[-3:].all() and not ref.bad[:-3].any()
    assert (ref.best_row[~fin] == -1).all() and np.isnan(ref.alive[:, ~fin]).all() and np.isnan(ref.count_prob[:, ~fin]).all()
    # count_prob rows sum to 1; alive is non-increasing in f and <= support
    assert np.allclose(ref.count_prob[:, fin].sum(-1), 1.0, rtol=0, atol=1e-12)
    assert (np.diff(ref.alive[:, fin], axis=0) <= 1e-15).all()
    assert (ref.alive[:, fin] <= ref.support[fin][None] + 1e-15).all()
    # what the generator must produce
    i = {n: g.names.index(n) for n in ("twin", "tiny", "fresh")}
    assert ref.best_row[i["fresh"]] >= 0 and not ref.presence[i["fresh"]].any() and not ref.support[i["fresh"]].any()
    if N > 1 and K > 1:   # two best-row objects follow one id in the odd particles
        m = ref.match[i["twin"]]
        assert ((m[1::2, 0] == 0) & (m[1::2, 1] == 0)).any()
    box = ref.box0[i["tiny"], 0]
    assert 0 < box[2] * box[3] < 1e-3                            # the degenerate box: the floor of to_coords, never exactly 0
    if F > 1:
        assert (ref.alive[-1, fin] < ref.alive[0, fin] - 1e-9).any()           # objects die ...
        assert K * S > 8 or np.isnan(ref.box_mean[:, fin]).any()               # ... some in every rollout (where they are few)
        moved = (ref.slot[0] >= 0) & (ref.slot[-1] >= 0) & (ref.slot[0] != ref.slot[-1])
        assert moved.any()                                                     # ids move between slots
    decisions, skip = FL.near_threshold(ref, iou_min)
    assert decisions > 0 and skip.sum() <= 0.01 * decisions, (decisions, int(skip.sum()))
