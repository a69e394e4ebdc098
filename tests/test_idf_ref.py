"""No GPU: the reference of IDF1 scoring (tests/idf_ref.py) against answers known by hand, its two solvers against each other, and --
from the reference alone -- that the inputs of tests/test_idf_kernel.py (tests/idf_cases.py) leave at most 1 % of the lanes fragile:
lanes on which a present pair's float64 IoU lies within four times the measured fp32 error of iou_min (tests/score_ref.py:
iou32_error; the factor covers the device's division, as in the score's test), left out from their first such frame on."""
import numpy as np
import pytest

from tests import idf_cases as IC
from tests import idf_ref as R
from tests import score_ref as SR

BOX = {"a": (5.0, 5.0, 10.0, 10.0), "b": (30.0, 30.0, 12.0, 12.0), "c": (5.0, 30.0, 8.0, 8.0), "far": (100.0, 100.0, 5.0, 5.0)}
I = {n: i for i, n in enumerate(R.TOTALS)}


def _words(ids):
    """Float ids as the int32 words the kernels compare."""
    return SR.words(np.asarray(ids, np.float32))


def _clip(frames, G, N, P, iou_min=0.5, table=None):
    """One lane.  ``frames``: per frame dict(truth={g: box name}, lane=[(box name, float id)], valid=True, finite=True).  Returns the
    table after, the score's reference (for idsw) and the inputs."""
    T = len(frames)
    x = dict(box=np.zeros((T, 1, N, 4), np.float32), presence=np.zeros((T, 1, N), np.float32), obj_id=np.zeros((T, 1, N), np.float32),
             map_count=np.zeros((T, 1), np.int32), truth_box=np.zeros((T, 1, G, 4), np.float32),
             truth_present=np.zeros((T, 1, G), np.int32), truth_valid=np.ones((T, 1), np.int32))
    for t, fr in enumerate(frames):
        for g, name in fr.get("truth", {}).items():
            x["truth_box"][t, 0, g], x["truth_present"][t, 0, g] = BOX[name], 1
        for j, (name, i) in enumerate(fr.get("lane", [])):
            x["box"][t, 0, j], x["presence"][t, 0, j], x["obj_id"][t, 0, j] = BOX[name], 1.0, i
        x["map_count"][t, 0] = len(fr.get("lane", [])) if fr.get("finite", True) else -1
        x["truth_valid"][t, 0] = int(fr.get("valid", True))
    sc = SR.score(iou_min=iou_min, **x)
    table = R.new_table(1, G, P) if table is None else table
    after = R.accumulate(table, x["box"], x["presence"], _words(x["obj_id"]), x["map_count"], x["truth_box"], x["truth_present"],
                         x["truth_valid"], sc.truth_match, iou_min)
    return after, sc, x


def _figures(table):
    fig, _ = R.figures(table, 0)
    fig_b, _ = R.figures(table, 0, R.best_brute)
    assert np.array_equal(fig, fig_b)
    return dict(zip(R.TOTALS, fig.tolist()))


def _idf1(f):
    return 2.0 * f["idtp"] / (2 * f["idtp"] + f["idfp"] + f["idfn"])


def test_one_truth_followed_by_id_1_then_id_2():
    frames = [dict(truth={0: "a"}, lane=[("a", 1.0)])] * 6 + [dict(truth={0: "a"}, lane=[("a", 2.0)])] * 4
    t, sc, _ = _clip(frames, 1, 1, 4)
    f = _figures(t)
    assert (f["idtp"], f["idfn"], f["idfp"], f["ids"], f["frames"], f["clips"], f["trajectories"]) == (6, 4, 4, 2, 10, 1, 1)
    assert _idf1(f) == 0.6 and int(sc.counts[0, 6]) == 1      # the score counts one switch
    assert (f["mt"], f["frag"], f["overflow_ids"]) == (1, 0, 0)
    # where the switch falls changes IDF1, not idsw
    early = [dict(truth={0: "a"}, lane=[("a", 1.0)])] * 1 + [dict(truth={0: "a"}, lane=[("a", 2.0)])] * 9
    t2, sc2, _ = _clip(early, 1, 1, 4)
    assert _idf1(_figures(t2)) == 0.9 and int(sc2.counts[0, 6]) == 1


def test_two_truths_whose_ids_swap_half_way():
    first = dict(truth={0: "a", 1: "b"}, lane=[("a", 1.0), ("b", 2.0)])
    second = dict(truth={0: "a", 1: "b"}, lane=[("a", 2.0), ("b", 1.0)])
    t, _, _ = _clip([first] * 5 + [second] * 5, 2, 2, 8)
    f = _figures(t)
    assert np.array_equal(R.masked_overlap(t, 0)[:, :2], [[5, 5], [5, 5]])
    assert (f["idtp"], f["idfn"], f["idfp"]) == (10, 10, 10) and _idf1(f) == 0.5


def test_greedy_gives_5_and_the_optimum_is_8():
    w = np.array([[5, 4], [4, 0]])
    greedy, left = 0, w.astype(np.int64).copy()
    while left.max() > 0:
        g, p = np.unravel_index(left.argmax(), left.shape)
        greedy += int(left[g, p])
        left[g, :], left[:, p] = 0, 0
    assert greedy == 5 and R.best_scipy(w)[0] == 8 and R.best_brute(w) == 8
    assert R.best_scipy(w)[1].tolist() == [1, 0]
    assert R.best_scipy(np.array([[-3, -1]]))[0] == 0 and R.best_brute(np.array([[-3, -1]])) == 0     # unassigned beats a negative pair
    assert R.best_scipy(np.array([[2], [7], [3]]))[0] == 7 and R.best_brute(np.array([[2], [7], [3]])) == 7   # more rows than columns


@pytest.mark.parametrize("gap", [(2, 4), (5, 7), (7, 9)])
def test_a_drop_out_bridged_under_the_same_id(gap):
    frames = [dict(truth={0: "a"}, lane=[] if gap[0] <= t < gap[1] else [("a", 7.0)]) for t in range(10)]
    t, sc, _ = _clip(frames, 1, 2, 4)
    f = _figures(t)
    assert (f["frag"], f["idtp"], f["idfn"], f["idfp"], f["ids"]) == (1, 8, 2, 0, 1) and int(sc.counts[0, 6]) == 0
    assert _idf1(f) == 16.0 / 18.0
    assert t["trk_state"][0, 0] == 3 and (f["mt"], f["pt"], f["ml"]) == (1, 0, 0)       # 8 of 10: exactly 80 %


@pytest.mark.parametrize("present, hit, cls", [(5, 4, "mt"), (10, 8, "mt"), (10, 7, "pt"), (5, 1, "pt"), (10, 2, "pt"), (10, 1, "ml"), (5, 0, "ml")])
def test_mostly_tracked_partly_tracked_mostly_lost_at_the_edges(present, hit, cls):
    frames = [dict(truth={0: "a"}, lane=[("a", 1.0)] if t < hit else [("far", 1.0)]) for t in range(present)]
    f = _figures(_clip(frames, 2, 1, 2)[0])
    assert {n: f[n] for n in ("mt", "pt", "ml")} == dict(dict(mt=0, pt=0, ml=0), **{cls: 1}) and f["trajectories"] == 1


def test_more_ids_than_columns():
    frames = [dict(truth={0: "a"}, lane=[("a", float(10 + t))]) for t in range(5)]
    t, _, _ = _clip(frames, 1, 1, 2)
    f = _figures(t)
    assert t["col_id"][0].tolist() == _words([10.0, 11.0]).tolist() and t["extra_frames"][0] == 3
    assert t["totals"][0, I["overflow_ids"]] == 3 and not R.pooled(t["totals"] + R.solve(t)[1])["exact"]
    assert (f["idtp"], f["idfn"], f["idfp"], f["ids"]) == (1, 4, 4, 2)          # IDFP carries the three unkeyed frames


def test_a_negative_id_word_and_a_repeated_word_are_unkeyed():
    frames = [dict(truth={0: "a", 1: "b"}, lane=[("a", -2.0), ("b", 3.0)])] * 2 + [dict(truth={0: "a", 1: "b"}, lane=[("a", 3.0), ("b", 3.0)])]
    t, _, _ = _clip(frames, 2, 2, 4)
    f = _figures(t)
    assert (t["col_id"][0] >= 0).sum() == 1 and t["extra_frames"][0] == 3 and t["totals"][0, I["overflow_ids"]] == 3
    assert np.array_equal(R.masked_overlap(t, 0)[:, 0], [1, 2]) and t["col_frames"][0, 0] == 3
    assert (f["idtp"], f["idfn"], f["idfp"]) == (2, 4, 4)


def test_an_invalid_frame_and_a_non_finite_lane_touch_nothing():
    good = dict(truth={0: "a"}, lane=[("a", 1.0)])
    t0, _, _ = _clip([good] * 3, 1, 1, 2)
    t1, _, _ = _clip([good, dict(good, valid=False), good, dict(good, finite=False), good], 1, 1, 2)
    assert all(np.array_equal(t0[n], t1[n]) for n in t0)


def test_close_then_reopen():
    a = [dict(truth={0: "a"}, lane=[("a", 1.0)])] * 4
    b = [dict(truth={0: "b"}, lane=[("b", 1.0)])] * 2 + [dict(truth={0: "b"}, lane=[("b", 5.0)])] * 1
    t, _, _ = _clip(a, 1, 1, 2)
    closed, open_ = R.solve(t, close=np.array([1]))
    assert open_[0].tolist() == [1, 4, 1, 4, 0, 0, 1, 0, 0, 0, 1, 0] and np.array_equal(closed["totals"][0], open_[0])
    assert (closed["col_id"] == -1).all() and not closed["row_frames"].any() and not closed["frames"].any()
    assert np.array_equal(closed["overlap"], t["overlap"])                      # stale words stay and are never read
    again, _, _ = _clip(b, 1, 1, 2, table=closed)
    assert again["overlap"][0, 0].tolist() == [2, 1] and again["col_frames"][0].tolist() == [2, 1]
    final, open2 = R.solve(again, close=np.array([1]))
    assert open2[0].tolist() == [1, 3, 1, 2, 1, 1, 1, 0, 0, 0, 2, 0]
    assert final["totals"][0].tolist() == [2, 7, 2, 6, 1, 1, 2, 0, 0, 0, 3, 0]
    assert R.pooled(final["totals"])["idf1"] == 12.0 / 14.0
    same, open3 = R.solve(again)                                                # without close nothing changes
    assert all(np.array_equal(same[n], again[n]) for n in again) and np.array_equal(open3, open2)
    empty, open4 = R.solve(R.new_table(1, 1, 2), close=np.array([1]))           # an empty clip is no clip
    assert not open4.any() and not empty["totals"].any() and np.isnan(R.pooled(open4)["idf1"])


def test_scipy_against_brute_force_on_small_tables():
    rng = np.random.default_rng(5)
    for trial in range(300):
        G, P = int(rng.integers(1, 6)), int(rng.integers(1, 7))
        w = rng.integers(0, (4, 1 << 20, 60)[trial % 3], (G, P)) * (rng.uniform(size=(G, P)) < (1.0, 1.0, 0.3)[trial % 3])
        best, r2c = R.best_scipy(w)
        assert best == R.best_brute(w), (trial, w)
        cols = r2c[r2c >= 0]
        assert len(set(cols.tolist())) == len(cols) and sum(int(w[g, p]) for g, p in enumerate(r2c) if p >= 0) == best


@pytest.mark.parametrize("i", range(len(IC.CASES)), ids=[IC.case_id(c) for c in IC.CASES])
def test_the_kernel_tests_inputs_leave_few_fragile_lanes_and_exercise_every_path(i):
    c = IC.CASES[i]
    x = IC.make(c)
    near = 4.0 * SR.iou32_error(x["truth_box"], x["box"])
    first = R.fragile_from(SR.iou_table(x["truth_box"], x["box"]), x["presence"], x["map_count"], x["truth_present"], x["truth_valid"],
                           c.iou_min, near)
    left_out = int((first < IC.T).sum())
    print(IC.case_id(c), "near", near, "lanes left out as fragile:", left_out, "of", IC.B)
    assert near < 1e-5 and left_out <= IC.FRAGILE_CAP * IC.B
    t = R.accumulate(R.new_table(IC.B, c.G, c.P), x["box"], x["presence"], x["ids"], x["map_count"], x["truth_box"], x["truth_present"],
                     x["truth_valid"], x["truth_match"], c.iou_min)
    _, open_ = R.solve(t)
    tot = dict(zip(R.TOTALS, (open_.sum(0) + t["totals"].sum(0)).tolist()))
    print(IC.case_id(c), tot)
    assert tot["idtp"] > 0 and tot["idfn"] > 0 and tot["idfp"] > 0 and tot["frag"] > 0 and tot["overflow_ids"] > 0
    assert tot["mt"] > 0 and tot["ml"] > 0 and (c.G == 1 or tot["pt"] > 0)
    if c.P < 2 * c.N:     # the overflowing cases: some lane sees more ids than columns
        assert ((t["col_id"] >= 0).all(1) & (t["extra_frames"] > 0)).any()
    if c.G <= 5 and c.P <= 6:
        for b in range(IC.B):
            assert R.figures(t, b)[0][I["idtp"]] == R.figures(t, b, R.best_brute)[0][I["idtp"]]
