"""No GPU: known answers of the float64 lane-estimate reference (tests/estimate_ref.py; the semantics: include/sqair_hip.h,
sqair_set_estimate) -- the thing the kernel and the stream are compared against has to be right on cases worked out by hand."""
import numpy as np
import pytest

from oracle import sqair_oracle as O
from tests import estimate_ref as E

HW = (50, 50)


def _where(yxhw, hw=HW):
    """where logits whose box is (y, x, h, w) pixels (the oracle's inverse maps), float32."""
    return O.to_logits(O.pixel_to_stn_coords(np.asarray(yxhw, dtype=np.float64), hw)).astype(np.float32)


def _scene(rows, N, hw=HW):
    """One frame: rows = per particle row a list of (y, x, h, w) boxes (present-first) -> where [1, R, N, 4], presence, obj_id."""
    R = len(rows)
    where = np.zeros((1, R, N, 4), np.float32)
    pres = np.zeros((1, R, N), np.float32)
    ids = np.full((1, R, N), -1.0, np.float32)
    for r, bxs in enumerate(rows):
        for j, bx in enumerate(bxs):
            where[0, r, j] = _where(bx, hw)
            pres[0, r, j] = 1.0
            ids[0, r, j] = 10 * r + j
    return where, pres, ids


A1, A2, B1 = (5.0, 5.0, 10.0, 10.0), (30.0, 8.0, 12.0, 9.0), (28.0, 35.0, 8.0, 8.0)   # pairwise disjoint


def test_box_is_the_references_pixel_box():
    # zero logits: sx = sy = 1/2, tx = ty = 0 -> y = (H - 1) / 4, h = (H + 1) / 2 (sqair/modules.py:246-262)
    assert np.allclose(E.boxes(np.zeros(4), (50, 30)), [49 / 4, 29 / 4, 51 / 2, 31 / 2], rtol=0, atol=1e-12)
    # and the inverse maps round-trip a pixel box through where logits (float32 logits: ~1e-6 pixels)
    assert np.allclose(E.boxes(_where(A2), HW), A2, rtol=0, atol=1e-4)
    # a scale logit far below zero is kept at 1e-4 (the clip of modules.py:205-206): h = (H + 1) 1e-4
    assert np.allclose(E.boxes(np.array([-40.0, -40.0, 0.0, 0.0]), HW)[2:], [51e-4, 51e-4], rtol=1e-12)


def test_iou_by_hand():
    assert E.iou((0, 0, 2, 2), (1, 1, 2, 2)) == pytest.approx(1.0 / 7.0, abs=1e-15)     # overlap 1, union 4 + 4 - 1
    assert E.iou((0, 0, 2, 4), (1, 2, 2, 4)) == pytest.approx(2.0 / 14.0, abs=1e-15)    # overlap 1 x 2, union 8 + 8 - 2
    assert E.iou((0, 0, 2, 2), (2, 0, 2, 2)) == 0.0                                     # touching edges
    assert E.iou((0, 0, 2, 2), (5, 5, 1, 1)) == 0.0                                     # disjoint
    assert E.iou((0, 0, 4, 4), (1, 1, 2, 2)) == pytest.approx(0.25, abs=1e-15)          # contained
    assert E.iou((0.1, 0.7, 3.3, 1.9), (0.1, 0.7, 3.3, 1.9)) == 1.0                     # the same four values: exactly 1
    assert E.iou((1, 1, 0, 0), (1, 1, 0, 0)) == 0.0                                     # the union is not positive


def test_one_particle():
    where, pres, ids = _scene([[A1, A2]], N=4)
    o = E.estimate(where, pres, ids, np.array([[-3.5]], np.float32), 1, HW, 0.5)
    assert o.weights[0, 0, 0] == 1.0 and o.ess[0, 0] == 1.0 and o.best_row[0, 0] == 0
    assert list(o.count_prob[0, 0]) == [0, 0, 1, 0, 0] and o.expected_count[0, 0] == 2 and o.map_count[0, 0] == 2
    assert list(o.support[0, 0]) == [1, 1, 0, 0]
    assert np.array_equal(o.box_mean[0, 0], o.box[0, 0]) and np.allclose(o.box[0, 0, :2], [A1, A2], atol=1e-4)
    assert np.array_equal(o.presence[0, 0], pres[0, 0]) and list(o.obj_id[0, 0]) == [0, 1, 0, 0]   # zero where absent
    assert np.array_equal(o.where[0, 0, :2], where[0, 0, :2]) and not o.where[0, 0, 2:].any() and not o.box[0, 0, 2:].any()


def test_identical_particles_have_full_support():
    K = 5
    where, pres, ids = _scene([[A1, B1]] * K, N=3)
    lw = np.random.default_rng(0).standard_normal((1, K)).astype(np.float32)
    o = E.estimate(where, pres, ids, lw, K, HW, 1.0)      # iou_min = 1: identical boxes still agree
    assert np.allclose(o.support[0, 0], [1, 1, 0], rtol=0, atol=1e-15)
    assert np.allclose(o.box_mean[0, 0], o.box[0, 0], rtol=0, atol=1e-12)
    assert o.best_row[0, 0] == int(np.argmax(lw[0])) and o.count_prob[0, 0, 2] == pytest.approx(1.0, abs=1e-15)


def test_two_groups_of_particles():
    # particles 0, 1 (weight 0.35 each) see A1 and A2; particles 2, 3 (0.15 each) see one object somewhere else
    where, pres, ids = _scene([[A1, A2], [A1, A2], [B1], [B1]], N=3)
    lw = np.log(np.array([[0.35, 0.35, 0.15, 0.15]])).astype(np.float32)
    o = E.estimate(where, pres, ids, lw, 4, HW, 0.5)
    assert o.best_row[0, 0] == 0
    assert np.allclose(o.weights[0, 0], [0.35, 0.35, 0.15, 0.15], atol=1e-7)
    assert np.allclose(o.support[0, 0], [0.7, 0.7, 0.0], atol=1e-7)
    assert np.allclose(o.count_prob[0, 0], [0, 0.3, 0.7, 0], atol=1e-7) and o.map_count[0, 0] == 2
    assert o.expected_count[0, 0] == pytest.approx(1.7, abs=1e-6)
    assert np.allclose(o.box_mean[0, 0, :2], [A1, A2], atol=1e-4)
    assert o.ess[0, 0] == pytest.approx(1.0 / (2 * 0.35 ** 2 + 2 * 0.15 ** 2), rel=1e-6)
    # the other way round: the minority's single object has support 0.3, and the frame before (prefix weights) differs
    lw2 = np.stack([-lw[0], 2 * lw[0]])                  # frame 0: the minority leads; frame 1: a = lw again
    w2, p2, i2 = (np.concatenate([x, x]) for x in (where, pres, ids))
    o = E.estimate(w2, p2, i2, lw2, 4, HW, 0.5)
    assert o.best_row[0, 0] == 2 and o.best_row[1, 0] == 0
    w0 = np.exp(-lw[0].astype(np.float64)) / np.exp(-lw[0].astype(np.float64)).sum()
    assert np.allclose(o.support[0, 0], [w0[2] + w0[3], 0, 0], atol=1e-7) and np.allclose(o.support[1, 0], [0.7, 0.7, 0], atol=1e-6)


def test_association_is_spatial_not_by_slot_or_id():
    # particle 1 holds the same two objects in the other order, with other ids: both still agree; matching is not one-to-one
    where, pres, ids = _scene([[A1, A2], [A2, A1], [A1]], N=2)
    o = E.estimate(where, pres, ids, np.zeros((1, 3), np.float32), 3, HW, 0.5)
    assert np.allclose(o.support[0, 0], [1.0, 2.0 / 3.0], atol=1e-12)
    assert list(o.match[0, 0, 1]) == [1, 0] and list(o.match[0, 0, 2]) == [0, -1]
    # a shifted copy agrees while its IoU stays above iou_min, and pulls the consensus box
    sh = (A1[0] + 2.0, A1[1], A1[2], A1[3])              # IoU = 8 / 12
    where, pres, ids = _scene([[A1], [sh]], N=2)
    for iou_min, sup in ((0.6, 1.0), (0.7, 0.5)):
        o = E.estimate(where, pres, ids, np.zeros((1, 2), np.float32), 2, HW, iou_min)
        assert o.iou_best[0, 0, 1, 0] == pytest.approx(8.0 / 12.0, abs=1e-5)
        assert o.support[0, 0, 0] == pytest.approx(sup, abs=1e-12)
        assert o.box_mean[0, 0, 0, 0] == pytest.approx(A1[0] + (1.0 if sup == 1.0 else 0.0), abs=1e-4)


def test_count_prob_sums_to_one():
    rng = np.random.default_rng(3)
    T, B, K, N = 2, 20, 7, 4
    where = rng.standard_normal((T, B * K, N, 4)).astype(np.float32)
    pres = (rng.uniform(size=(T, B * K, N)) < 0.5).astype(np.float32)
    o = E.estimate(where, pres, np.zeros_like(pres), rng.standard_normal((T, B * K)).astype(np.float32) * 3, K, HW, 0.5,
                   lw0=rng.standard_normal(B * K).astype(np.float32))
    assert np.allclose(o.count_prob.sum(-1), 1.0, atol=1e-12) and np.allclose(o.weights.sum(-1), 1.0, atol=1e-12)
    assert np.allclose(o.expected_count, (o.count_prob * np.arange(N + 1)).sum(-1), atol=1e-12)
    assert ((o.support >= 0) & (o.support <= 1 + 1e-12)).all()
    # the best row always agrees with itself: the support of a present object is at least the best row's weight
    wb = np.take_along_axis(o.weights, (o.best_row % K)[..., None], -1)
    assert (o.support >= np.where(o.presence != 0, wb, 0.0) - 1e-12).all()


def test_first_of_maximal_on_exact_ties():
    # equal weights: the first row; count_prob[0] = count_prob[1] = 1/2: the first count; two identical slots: the first slot
    where, pres, ids = _scene([[A1], []], N=2)
    o = E.estimate(where, pres, ids, np.full((1, 2), -1.25, np.float32), 2, HW, 0.5)
    assert o.best_row[0, 0] == 0 and list(o.count_prob[0, 0]) == [0.5, 0.5, 0.0] and o.map_count[0, 0] == 0
    where, pres, ids = _scene([[], [A1]], N=2)
    o = E.estimate(where, pres, ids, np.full((1, 2), -1.25, np.float32), 2, HW, 0.5)
    assert o.best_row[0, 0] == 0 and o.map_count[0, 0] == 0 and not o.presence.any() and not o.support.any()
    where, pres, ids = _scene([[A1], [A1, A1], [B1, A1, A1]], N=3)
    o = E.estimate(where, pres, ids, np.array([[0.0, -1.0, -1.0]], np.float32), 3, HW, 0.5)
    assert list(o.match[0, 0, :, 0]) == [0, 0, 1]
    # a later row that is larger by one fp32 ulp wins; frames accumulate in fp32
    lw = np.array([[1.0, np.nextafter(np.float32(1.0), np.float32(2.0))]], np.float32)
    assert E.estimate(where[:, :2], pres[:, :2], ids[:, :2], lw, 2, HW, 0.5).best_row[0, 0] == 1
    lw = np.array([[1.0, 1.0], [3e-8, 0.0]], np.float32)     # 1 + 3e-8 rounds to 1 in fp32: still a tie, the first row
    assert list(E.estimate(np.concatenate([where[:, :2]] * 2), np.concatenate([pres[:, :2]] * 2), np.concatenate([ids[:, :2]] * 2),
                           lw, 2, HW, 0.5).best_row[:, 0]) == [0, 0]


@pytest.mark.parametrize("kind", ["nan", "pos_inf", "all_neg_inf"])
def test_non_finite_lanes(kind):
    K, N = 3, 2
    where, pres, ids = _scene([[A1]] * (2 * K), N=N)
    lw0 = np.zeros((2, K), np.float32)
    lw0[1] = [0.0, -1.0, -np.inf]                           # a finite lane next to it (one particle at -inf is fine)
    lw0[0] = dict(nan=[0.0, np.nan, 0.0], pos_inf=[0.0, np.inf, 0.0], all_neg_inf=[-np.inf] * 3)[kind]
    canvas = np.ones((1, 2 * K, 4, 4))
    o = E.estimate(where, pres, ids, np.zeros((1, 2 * K), np.float32), K, HW, 0.5, lw0=lw0.reshape(-1), canvas=canvas)
    assert o.bad[0, 0] and not o.bad[0, 1]
    for name in ("weights", "ess", "count_prob", "expected_count", "support", "box_mean", "mean_canvas"):
        assert np.isnan(getattr(o, name)[0, 0]).all(), name
        assert np.isfinite(getattr(o, name)[0, 1]).all(), name
    assert o.best_row[0, 0] == -1 and o.map_count[0, 0] == -1
    for name in ("presence", "obj_id", "where", "box"):     # zero objects
        assert not getattr(o, name)[0, 0].any(), name
    assert o.best_row[0, 1] == K and o.support[0, 1, 0] == pytest.approx(1.0, abs=1e-15) and o.weights[0, 1, 2] == 0.0
    assert np.allclose(o.mean_canvas[0, 1], 1.0, atol=1e-15)
