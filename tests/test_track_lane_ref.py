"""No GPU: the float64 reference of the lane tracks (tests/track_lane_ref.py) against known answers, the properties the header states,
what the generator of the GPU test's inputs must produce, and the condition on those inputs: for its exact seeds, association
decisions within 1e-5 of the threshold (or of a tie) are at most 1 % of all decisions.  A condition the generator meets, not a
tolerance."""
import numpy as np
import pytest

from tests import estimate_ref as E
from tests import forecast_lane_check as FC
from tests import track_lane_check as TC
from tests import track_lane_ref as TL

HW = (50, 50)


def _one(where, pres, ids, valid, K, lw=None, iou_min=0.5):
    f32 = np.float32
    return TL.lane_tracks(np.asarray(where, f32), np.asarray(pres, f32), np.asarray(ids, f32), np.asarray(valid, np.int32), lw, K, HW, iou_min)


def test_single_path_is_its_own_answer():
    """K = 1: box_mean = the path's box, box_std = 0, alive in {0, 1}.  Object 7 sits in slot 1 at the newest frame and in slot 0 one
    frame earlier (compaction moved it); object 3 was born at the newest frame; the oldest frame is invalid."""
    rng = np.random.default_rng(0)
    where = rng.standard_normal((3, 1, 2, 4))
    pres = [[[1, 1]], [[1, 0]], [[1, 1]]]
    ids = [[[7.0, 9.0]], [[7.0, -1.0]], [[3.0, 7.0]]]
    o = _one(where, pres, ids, [[0], [1], [1]], 1)
    assert o.best_row[0] == 0 and (o.support == 1).all() and (o.weights == 1).all()
    assert np.array_equal(o.obj_id[0], [3.0, 7.0]) and np.array_equal(o.first_frame[0], [2, 1])
    assert np.array_equal(o.alive[:, 0], [[0, 0], [0, 1], [1, 1]])
    bx = E.boxes(where.astype(np.float32), HW)
    assert np.array_equal(o.box_mean[2, 0], bx[2, 0]) and np.array_equal(o.box_mean[1, 0, 1], bx[1, 0, 0])   # id 7 was in slot 0
    assert (o.box_std[2, 0] == 0).all() and (o.box_std[1, 0, 1] == 0).all()
    assert np.isnan(o.box_mean[1, 0, 0]).all() and np.isnan(o.box_std[0, 0]).all()
    # the invalid frame counts nowhere: not even as "zero objects"
    assert np.array_equal(o.count_prob[:, 0], [[0, 0, 0], [0, 1, 0], [0, 0, 1]]) and np.array_equal(o.valid_mass[:, 0], [0, 1, 1])
    # the same frame, valid: the path reaches back, id 7 is found there and first_frame moves with it
    o = _one(where, pres, ids, [[1], [1], [1]], 1)
    assert np.array_equal(o.first_frame[0], [2, 0]) and np.array_equal(o.alive[:, 0], [[0, 1], [0, 1], [1, 1]])
    assert np.array_equal(o.count_prob[0, 0], [0, 0, 1])


def test_two_paths_by_hand():
    """K = 2, weights 3 : 1, one object: the weighted mean and spread at the newest frame; one frame back the second path has ended, so
    the first is left alone with alive = valid_mass = its weight; an invalid best row gives no objects at all."""
    where = np.zeros((2, 2, 1, 4))
    where[1, 1, 0, 2] = 0.2                                       # the second particle's newest box, moved in x
    where[0, 0, 0, 3] = -0.4
    lw = np.log(np.array([3.0, 1.0], np.float32))
    o = _one(where, np.ones((2, 2, 1)), [[[4.0], [9.0]], [[4.0], [9.0]]], [[1, 0], [1, 1]], 2, lw=lw)
    bx = E.boxes(where.astype(np.float32), HW)[:, :, 0]
    w = o.weights[0]
    assert np.allclose(w, [0.75, 0.25], atol=1e-7) and o.best_row[0] == 0 and o.support[0, 0] == 1.0
    mean = w[0] * bx[1, 0] + w[1] * bx[1, 1]
    assert np.allclose(o.box_mean[1, 0, 0], mean, atol=1e-12)
    assert np.allclose(o.box_std[1, 0, 0], np.sqrt(w[0] * (bx[1, 0] - mean) ** 2 + w[1] * (bx[1, 1] - mean) ** 2), atol=1e-12)
    assert o.box_std[1, 0, 0, 1] > 1.0
    assert np.isclose(o.alive[0, 0, 0], w[0]) and np.isclose(o.valid_mass[0, 0], w[0]) and o.valid_mass[1, 0] == 1.0
    assert np.allclose(o.box_mean[0, 0, 0], bx[0, 0]) and (o.box_std[0, 0, 0] < 1e-12).all()
    assert np.allclose(o.count_prob[:, 0], [[0, w[0]], [0, 1.0]]) and o.first_frame[0, 0] == 0
    # the best row's newest frame is invalid (an empty path): a lane without objects, and the other particle associates with nothing
    o = _one(where, np.ones((2, 2, 1)), [[[4.0], [9.0]], [[4.0], [9.0]]], [[0, 1], [0, 1]], 2, lw=lw)
    assert o.best_row[0] == 0 and not o.presence.any() and not o.support.any() and not o.alive.any() and (o.first_frame == -1).all()
    assert np.allclose(o.valid_mass[:, 0], w[1]) and np.allclose(o.count_prob[:, 0, 1], w[1])


@pytest.mark.parametrize("case", TL.CASES, ids=[TL.case_id(c) for c in TL.CASES])
def test_gpu_cases_properties_and_threshold_cap(case):
    K, F, N, wide, hw, iou_min = case
    g = TL.make_paths(case)
    ref = TL.lane_tracks(g.where, g.presence, g.obj_id, g.valid, g.log_w, K, hw, iou_min)
    fin = ~ref.bad
    assert ref.bad[-3:].all() and not ref.bad[:-3].any()
    assert (ref.best_row[~fin] == -1).all() and np.isnan(ref.alive[:, ~fin]).all() and np.isnan(ref.count_prob[:, ~fin]).all()
    assert np.isnan(ref.valid_mass[:, ~fin]).all() and (ref.first_frame[~fin] == -1).all()
    # count_prob sums to valid_mass; alive[F - 1] is the support; alive is non-decreasing in f (an id's presence along a path is one
    # interval ending at F - 1, in these inputs as in a stream) and <= min(support, valid_mass)
    assert np.allclose(ref.count_prob[:, fin].sum(-1), ref.valid_mass[:, fin], rtol=0, atol=1e-12)
    assert np.array_equal(ref.alive[F - 1, fin], ref.support[fin])
    assert (np.diff(ref.alive[:, fin], axis=0) >= -1e-15).all()
    assert (ref.alive[:, fin] <= np.minimum(ref.support[fin][None], ref.valid_mass[:, fin, None]) + 1e-15).all()
    assert (np.diff(ref.valid_mass[:, fin], axis=0) >= -1e-15).all() and (ref.valid_mass[:, fin] <= 1 + 1e-12).all()
    present = ref.presence != 0
    assert ((ref.first_frame >= 0) == present).all() and (ref.first_frame < F).all()
    # the reference is the comparison's fixed point: held against itself it passes with every margin 0
    as_got = {n: np.asarray(getattr(ref, n)) for n in ("best_row", "weights", "obj_id", "presence", "box0", "support", "first_frame",
                                                      "alive", "box_mean", "box_std", "count_prob", "valid_mass")}
    margins, counts = TC.check(as_got, ref, g.where, g.presence, g.valid, K, hw, iou_min)
    assert max(margins.values()) == 0 and counts["stats_checked"] > 0
    # what the generator must produce
    i = {n: g.names.index(n) for n in ("twin", "tiny", "fresh")}
    assert ref.best_row[i["fresh"]] >= 0 and not present[i["fresh"]].any() and not ref.support[i["fresh"]].any()
    if N > 1 and K > 1:   # two best-row objects follow one id in the odd particles
        m = ref.match[i["twin"]]
        assert ((m[1::2, 0] == 0) & (m[1::2, 1] == 0)).any()
    box = ref.box0[i["tiny"], 0]
    assert 0 < box[2] * box[3] < 1e-3                            # the degenerate box: the floor of to_coords, never exactly 0
    valid = g.valid.reshape(F, g.B, K)
    if F > 1:
        assert (ref.alive[0, fin] < ref.alive[-1, fin] - 1e-9).any()           # objects born inside the window ...
        assert K > 8 or np.isnan(ref.box_mean[:, fin]).any()                   # ... some in every path (where they are few)
        moved = (ref.slot[0] >= 0) & (ref.slot[-1] >= 0) & (ref.slot[0] != ref.slot[-1])
        assert moved.any()                                                     # ids move between slots
        assert (valid[0] == 0).any() and (valid[0] < valid[-1]).any()          # paths that end fresh inside the window
        assert (present & (ref.first_frame > 0)).any() and (present & (ref.first_frame == 0)).any()
        assert (g.presence[g.valid == 0] != 0).any() and not g.presence.reshape(F, g.B, K, N)[:, 0::3][valid[:, 0::3] == 0].any()
    if F > 1 and K > 1:    # coalesced genealogies: older frames of distinct particles are word-for-word the same row
        assert g.coalesced.any()
        w0 = g.where.reshape(F, g.B, K, N, 4)[0]
        assert any(len({w0[b, k].tobytes() for k in range(K)}) < K for b in np.flatnonzero(g.coalesced))
        assert (g.where.reshape(F, g.B, K, N, 4)[:, g.coalesced].std(2) > 0).any()      # ... and the newer ones are not
    if K > 1:
        assert (valid[-1] == 0).any()                                          # empty paths: a row invalid even at the newest frame
    decisions, skip = TL.near_threshold(ref, iou_min)
    assert decisions > 1 and skip.sum() <= 0.01 * decisions, (decisions, int(skip.sum()))
