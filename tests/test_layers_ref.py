"""No GPU: the float64 reference of the object layers (tests/layers_ref.py) against the oracle's decoder and the header's rules, and
the kernel cases (tests/layers_cases.py) against the cap on near-threshold decisions that tests/test_layers_kernel.py holds the
device to."""
import numpy as np
import pytest
import torch

from oracle import sqair_oracle as O
from tests import layers_cases as LC
from tests import layers_ref as L


def test_k1_recomposes_the_oracles_canvas():
    """At K = 1 layer[j] = V(best, j): sum_j layer[j] + mean_img * sigmoid(-10 + 20 sum_j cover[j]) is the decoder's canvas of the row
    (AIRDecoder._decode, as the oracle's decode and tests/test_hip_kernels.py::test_st_insert_loglik form it)."""
    c = LC.CASES[0]
    assert c.K == 1
    x = LC.make(c)
    H, W = c.hw
    ref = L.layers(x["glimpse"], x["where"], x["presence"], x["lw"], 1, c.hw, LC.IOU_MIN, LC.COVER_MIN, lw0=x["lw0"])
    mean_img = np.random.default_rng(0).uniform(size=c.hw)
    R, N, G = x["B"], c.N, c.G
    D = torch.float64
    g = torch.tensor(x["glimpse"][0], dtype=D).reshape(R * N, G, G)
    wl = torch.tensor(x["where"][0], dtype=D).reshape(R * N, 4)
    p = torch.tensor(x["presence"][0], dtype=D)[..., None, None]
    inv = O.st_insert(g, wl, H, W).reshape(R, N, H, W) * p
    nz = torch.sigmoid(-10.0 + 20.0 * (O.st_insert(torch.ones_like(g), wl, H, W).reshape(R, N, H, W) * p).sum(1))
    canvas = (inv.sum(1) + torch.tensor(mean_img)[None] * nz).numpy()
    fin = ~ref.bad[0]
    assert fin.sum() == c.lanes and ref.present[0][fin].any()
    got = ref.layer[0].sum(1) + mean_img[None] * (1.0 / (1.0 + np.exp(10.0 - 20.0 * ref.cover[0].sum(1))))
    assert np.abs(got[fin] - canvas[fin]).max() <= 1e-12
    # a single particle agrees with itself on every object, with the slot itself
    assert np.array_equal(ref.match[0, fin, 0], np.where(ref.present[0][fin], np.arange(N)[None], -1))
    assert np.isnan(ref.layer[0][~fin]).all() and (ref.match[0][~fin] == -1).all() and (ref.owner[0][~fin] == -1).all()


def test_owner_rule_on_hand_made_covers():
    cover = np.zeros((5, 1, 4), np.float32)          # [N = 5, H = 1, W = 4]
    present = np.array([True, True, False, True, True])
    cover[:, 0, 0] = [0.7, 0.7, 0.9, 0.6, 0.7]       # ties: the first of the maximal present ones; an absent one never counts
    cover[:, 0, 1] = [0.1, 0.49999, 1.0, 0.3, 0.2]   # below cover_min: background
    cover[:, 0, 2] = [np.nan, 0.5, 0.0, np.nan, 0.2] # a NaN never wins; exactly cover_min does
    cover[:, 0, 3] = [np.nan, np.nan, 0.8, np.nan, np.nan]
    assert L.owner_rule(cover, present, 0.5).tolist() == [[0, -1, 1, -1]]
    assert L.owner_rule(cover.astype(np.float64), present, 0.5).tolist() == [[0, -1, 1, -1]]
    assert L.owner_rule(cover, np.zeros(5, bool), 0.5).tolist() == [[-1, -1, -1, -1]]
    assert L.owner_rule(cover, present, 0.75).tolist() == [[-1, -1, -1, -1]]
    # leading dimensions broadcast: [T, B, N, H, W] with [T, B, N]
    both = L.owner_rule(np.stack([cover, cover[::-1]])[None], np.stack([present, present[::-1]])[None], 0.5)
    assert both.shape == (1, 2, 1, 4) and both[0, 0].tolist() == [[0, -1, 1, -1]] and both[0, 1].tolist() == [[0, -1, 3, -1]]


def test_a_given_match_table_replaces_the_references_own():
    c = LC.CASES[2]
    x = LC.make(c)
    args = (x["glimpse"], x["where"], x["presence"], x["lw"], c.K, c.hw, LC.IOU_MIN, LC.COVER_MIN)
    own = L.layers(*args, lw0=x["lw0"])
    again = L.layers(*args, lw0=x["lw0"], match=own.match)
    assert np.array_equal(own.layer, again.layer, equal_nan=True) and np.array_equal(own.owner, again.owner)
    # only the best row kept: the layer of an object is then the best row's own V, its support the best row's weight
    est = own.est
    kb = np.where(est.bad, 0, est.best_row % c.K)
    only = np.full_like(own.match, -1)
    t, b = np.indices(kb.shape)
    only[t, b, kb] = own.match[t, b, kb]
    alone = L.layers(*args, lw0=x["lw0"], match=only)
    V, _ = L.slot_images(x["glimpse"], x["where"], x["presence"], c.hw)
    V = V.reshape((c.T, x["B"], c.K, c.N) + c.hw)
    seen = 0
    for bb in np.flatnonzero(~est.bad[0]):
        for j in np.flatnonzero(own.present[0, bb]):
            assert np.abs(alone.layer[0, bb, j] - V[0, bb, kb[0, bb], own.match[0, bb, kb[0, bb], j]]).max() <= 1e-12
            assert abs(alone.support[0, bb, j] - est.weights[0, bb, kb[0, bb]]) <= 1e-15
            assert own.support[0, bb, j] == est.support[0, bb, j]
            seen += 1
    assert seen > 20
    # absent objects are zero, and a convex combination of covers stays in [0, 1]
    assert not own.layer[~own.bad][~own.present[~own.bad]].any() and not own.cover[~own.bad][~own.present[~own.bad]].any()
    fin = own.cover[~own.bad]
    assert fin.min() >= 0.0 and fin.max() <= 1.0 + 1e-12 and fin.max() > 0.9


@pytest.mark.parametrize("c", LC.CASES, ids=[LC.case_id(c) for c in LC.CASES])
def test_near_threshold_decisions_stay_under_the_cap(c):
    """The count the GPU test caps, from the reference alone: at most 1 % of the association decisions of a case lie within 1e-5 of
    a threshold.  Also what the case is there for: lanes that agree and lanes that do not, owners and background."""
    x = LC.make(c)
    assert 11 <= x["B"] <= 48
    ref = L.layers(x["glimpse"], x["where"], x["presence"], x["lw"], c.K, c.hw, LC.IOU_MIN, LC.COVER_MIN, lw0=x["lw0"])
    near, decisions = L.near_decisions(ref.est, LC.IOU_MIN)
    print(LC.case_id(c), "decisions", decisions, "near", int(near.sum()))
    assert decisions > 0 and near.sum() <= 0.01 * decisions
    assert ref.bad[:, -3:].all() and not ref.bad[:, :-3].any()
    agree = ref.est.agree
    assert agree.any() and (c.K == 1 or (~agree & (ref.est.iou_best >= 0)).any())
    fin = ~ref.bad
    assert (ref.owner[fin] >= 0).any() and (ref.owner[fin] == -1).any()
    assert ref.present[fin].any() and not ref.present[fin].all()
