"""The presence-pattern classifier of tests/presence_patterns.py on hand-written layouts (CPU)."""
import numpy as np
import pytest

from tests import presence_patterns as PP


def _one(prev, prop, disc):
    """One (frame, row) cell; returns the set of pattern names that hold (hole_before_last cannot: T = 1)."""
    a = lambda v: np.asarray(v, np.float32).reshape(1, 1, -1)
    c = PP.classify(a(prop), a(disc), a(prev))
    return {k for k, v in c.items() if v[0, 0]}


@pytest.mark.parametrize("prev,prop,disc,want", [
    # nothing there, nothing found
    ([0, 0, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], {"empty"}),
    # identity: every object kept, one discovery appended
    ([1, 1, 0, 0], [1, 1, 0, 0], [1, 0, 0, 0], set()),
    # the LAST object dropped: a drop, but nobody moves
    ([1, 1, 1, 0], [1, 1, 0, 0], [0, 0, 0, 0], {"drop"}),
    # the first dropped, one survivor behind it
    ([1, 1, 0, 0], [0, 1, 0, 0], [0, 0, 0, 0], {"drop", "hole"}),
    # two dropped ahead of a survivor
    ([1, 1, 1, 0], [0, 0, 1, 0], [0, 0, 0, 0], {"drop", "hole", "two_holes"}),
    # two separate holes, each survivor with ONE absent slot ahead ... and the last with two
    ([1, 1, 1, 1], [0, 1, 0, 1], [0, 0, 0, 0], {"drop", "hole", "two_holes"}),
    # hole + discovery
    ([1, 1, 1, 0], [1, 0, 1, 0], [1, 0, 0, 0], {"drop", "hole", "hole_and_disc"}),
    # hole + discoveries that overflow and fill the row
    ([1, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 0], {"drop", "hole", "hole_and_disc", "overflow", "full"}),
    # full without overflow
    ([1, 1, 0, 0], [1, 1, 0, 0], [1, 1, 0, 0], {"full"}),
    # everything dropped, row empty
    ([1, 1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 0], {"drop", "all_dropped", "empty"}),
    # everything dropped, one rediscovered (N = 1)
    ([1], [0], [1], {"drop", "all_dropped", "full"}),
    ([1], [1], [1], {"overflow", "full"}),
    # a discovery pattern that is not a prefix is counted like any other
    ([1, 1, 0], [0, 1, 0], [0, 1, 1], {"drop", "hole", "hole_and_disc", "full"}),
])
def test_hand_written_cells(prev, prop, disc, want):
    assert _one(prev, prop, disc) == want


def test_counts_over_frames_rows_and_the_last_frame_rule():
    T, R, N = 3, 2, 3
    prev = np.zeros((T, R, N)); prop = np.zeros((T, R, N)); disc = np.zeros((T, R, N))
    # row 0: discovers two at t = 0, loses the first at t = 1 (hole, not in the last frame), keeps the survivor at t = 2
    disc[0, 0] = [1, 1, 0]
    prev[1, 0] = [1, 1, 0]; prop[1, 0] = [0, 1, 0]
    prev[2, 0] = [1, 0, 0]; prop[2, 0] = [1, 0, 0]
    # row 1: discovers three at t = 0, keeps them at t = 1, a hole only in the LAST frame
    disc[0, 1] = [1, 1, 1]
    prev[1, 1] = [1, 1, 1]; prop[1, 1] = [1, 1, 1]; disc[1, 1] = [1, 0, 0]
    prev[2, 1] = [1, 1, 1]; prop[2, 1] = [1, 0, 1]
    pat = PP.classify(prop, disc, prev)
    c = PP.count(pat)
    assert c["cells"] == 6
    assert c["hole"] == 2 and c["hole_before_last"] == 1 and pat["hole_before_last"][1, 0] and not pat["hole_before_last"][2, 1]
    assert c["drop"] == 2 and c["overflow"] == 1 and c["full"] == 2 and c["empty"] == 0 and c["all_dropped"] == 0
    assert c["two_holes"] == 0 and c["hole_and_disc"] == 0
    for k in PP.PATTERNS:
        assert pat[k].shape == (T, R) and pat[k].dtype == bool
    assert all(k in PP.table(c) for k in PP.PATTERNS)


def test_classifier_agrees_with_a_per_cell_loop():
    """The vectorised classifier against the definitions spelled out slot by slot, on random layouts."""
    rng = np.random.default_rng(0)
    T, R, N = 4, 50, 5
    prev = (rng.uniform(size=(T, R, N)) < 0.6).astype(np.float32)
    prev = -np.sort(-prev, -1)                                   # merged layouts are present-first
    prop = prev * (rng.uniform(size=(T, R, N)) < 0.6)
    disc = (rng.uniform(size=(T, R, N)) < 0.3).astype(np.float32)
    pat = PP.classify(prop, disc, prev)
    for t in range(T):
        for r in range(R):
            ahead = [int(sum(1 - prop[t, r, :j])) for j in range(N)]
            hole = any(prop[t, r, j] and ahead[j] >= 1 for j in range(N))
            n = int(prop[t, r].sum() + disc[t, r].sum())
            want = dict(drop=any(prev[t, r, j] and not prop[t, r, j] for j in range(N)), hole=hole,
                        two_holes=any(prop[t, r, j] and ahead[j] >= 2 for j in range(N)),
                        hole_and_disc=hole and disc[t, r].sum() >= 1, overflow=n > N, full=n >= N, empty=n == 0,
                        all_dropped=prev[t, r].sum() > 0 and prop[t, r].sum() == 0, hole_before_last=hole and t < T - 1)
            assert {k: bool(pat[k][t, r]) for k in PP.PATTERNS} == want, (t, r)
    assert PP.count(pat)["hole"] > 20 and PP.count(pat)["two_holes"] > 5


def test_require_passes_and_fails_with_the_whole_table():
    prev = np.array([[[1, 1, 0]]]); prop = np.array([[[0, 1, 0]]]); disc = np.array([[[1, 0, 0]]])
    c = PP.count(PP.classify(prop, disc, prev))
    assert PP.require(c, hole=1, hole_and_disc=1, drop=1) is c
    with pytest.raises(AssertionError) as e:
        PP.require(c, hole=1, overflow=1, all_dropped=2)
    msg = str(e.value)
    assert "'overflow': (0, 1)" in msg and "'all_dropped': (0, 2)" in msg and "'hole'" not in msg.split(";")[0]
    assert all("{}=".format(k) in msg for k in PP.PATTERNS) and "1 (frame, row) cells" in msg
    with pytest.raises(AssertionError, match="unknown pattern"):
        PP.require(c, holes=1)


def test_shapes_must_agree_and_torch_tensors_are_taken():
    import torch
    a = torch.zeros(2, 3, 4)
    assert PP.count(PP.classify(a, a, a))["empty"] == 6
    with pytest.raises(AssertionError):
        PP.classify(np.zeros((2, 3, 4)), np.zeros((2, 3, 4)), np.zeros((2, 3, 3)))


def test_moved_ids_follow_the_object():
    ids = np.array([[[1, 2, 3]], [[2, 3, -1]], [[2, 4, -1]], [[4, -1, -1]]], np.float32)   # [T = 4, R = 1, N = 3]
    mv = PP.moved_ids(ids)
    assert mv.shape == ids.shape and not mv[0].any()
    assert mv[1, 0].tolist() == [True, True, False]      # objects 2, 3 moved one slot forward
    assert mv[2, 0].tolist() == [False, False, False]    # 2 stays, 4 is new
    assert mv[3, 0].tolist() == [True, False, False]     # 4 moved from slot 1 to slot 0
