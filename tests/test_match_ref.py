"""The float64 reference of keep + optimal matching (tests/match_ref.py) held to what can be known without a GPU: SciPy's assignment
against brute force over all partial assignments for every table shape up to 5 x 5, the answers known by hand (tests/match_cases.py:
hand), and the two conditions the inputs of tests/test_match_kernel.py must meet from the reference alone -- in every case with
G, N >= 2 greedy and optimal differ in at least one scored frame in ten (a case that does not tell them apart tests nothing), and at
most 1 % of the lanes are left out for a candidate IoU within 1e-5 of iou_min.  Also measured here: e, the largest error of an fp32
restatement of sq_box_iou on these inputs in units of 2^-20, which the GPU test's slack on the sum of q is made of.  With
SQAIR_PARITY_DIR set the figures are added to match_parity.json there (the copy under profiles/ is such a file)."""
import numpy as np
import pytest

from tests import identity_ref as I
from tests import match_cases as MC
from tests import match_ref as M
from tests import score_ref as R
from tests import traj_score_ref as TR

IDS = [MC.case_id(c) for c in MC.CASES]


@pytest.mark.parametrize("G", range(1, 6))
@pytest.mark.parametrize("N", range(1, 6))
def test_scipy_finds_the_optimum_of_every_partial_assignment(G, N):
    rng = np.random.default_rng(10 * G + N)
    for k in range(60):
        kind = k % 4
        if kind == 0:      # the header's table: BIG + q or -1
            iou = rng.uniform(0.0, 1.0, (G, N))
            w = np.where(rng.uniform(size=(G, N)) < 0.6, M.BIG + M.q_of(iou), -1)
        elif kind == 1:    # small weights with many ties and zeros
            w = rng.integers(-1, 4, (G, N))
        elif kind == 2:    # nothing eligible in some rows and columns
            w = np.where(rng.uniform(size=(G, N)) < 0.3, M.BIG + rng.integers(0, 1 << 20, (G, N)), -1)
            w[rng.integers(0, G)] = -1
        else:              # every pair eligible, nearly equal
            w = M.BIG + (1 << 19) + rng.integers(-3, 4, (G, N))
        w = w.astype(np.int64)
        value, pairs = M.solve(w)
        assert value == M.solve_brute(w), (w, pairs)
        assert len({g for g, _ in pairs}) == len(pairs) == len({j for _, j in pairs}) and all(w[g, j] > 0 for g, j in pairs)
        assert value == sum(int(w[g, j]) for g, j in pairs)
        if kind in (0, 2, 3):   # cardinality first: the value's multiple of BIG is the largest number of eligible pairs
            card = M.solve_brute(np.where(w >= 0, 1, -1))
            assert len(pairs) == card == value >> 25


def test_q_is_the_iou_in_units_of_two_to_the_minus_twenty_rounded_to_even():
    assert M.q_of([0.0, 1.0, 0.5, 2.5 / M.UNIT, 3.5 / M.UNIT, 0.6]).tolist() == [0, 1 << 20, 1 << 19, 2, 4, 629146]
    assert 16 * (1 << 20) < M.BIG and M.BIG + (1 << 20) < 1 << 30          # cardinality dominates; the solver's exact range


def test_the_table_of_the_issue_and_the_sum_at_equal_cardinality():
    yes, none = np.ones(2, bool), -np.ones(2, np.int64)
    ids = np.array([5, 6])
    iou = np.array([[0.60, 0.54], [0.54, 0.08]])
    g, _ = R.assign(iou, yes, yes, ids, none, 0.5)
    o, claimed = M.assign(iou, yes, yes, ids, none, 0.5)
    assert g.tolist() == [0, -1] and o.tolist() == [1, 0] and claimed.all()
    iou = np.array([[0.9, 0.8], [0.85, 0.5]])
    g, _ = R.assign(iou, yes, yes, ids, none, 0.5)
    o, _ = M.assign(iou, yes, yes, ids, none, 0.5)
    total = lambda m: sum(iou[r, m[r]] for r in range(2))
    assert g.tolist() == [0, 1] and abs(total(g) - 1.40) < 1e-12 and o.tolist() == [1, 0] and abs(total(o) - 1.65) < 1e-12
    # keep wins: truth 0 remembers the id of object 0, and the kept pair costs the second pair
    iou = np.array([[0.60, 0.54], [0.54, 0.08]])
    o, claimed = M.assign(iou, yes, yes, ids, np.array([5, -1]), 0.5)
    assert o.tolist() == [0, -1] and claimed.tolist() == [True, False]
    # an absent row or column has no eligible pair, a NaN never passes, and a frame without an eligible pair matches nothing
    o, _ = M.assign(iou, np.array([True, False]), yes, ids, none, 0.5)
    assert o.tolist() == [0, -1]
    o, _ = M.assign(np.array([[np.nan, 0.54], [0.54, 0.08]]), yes, yes, ids, none, 0.5)
    assert o.tolist() == [1, 0]
    o, claimed = M.assign(iou, yes, yes, ids, none, 0.7)
    assert o.tolist() == [-1, -1] and not claimed.any()


def test_the_hand_cases():
    x, last, expect, greedy = MC.hand()
    opt = M.score(iou_min=MC.HAND_IOU, last_id=last, **x)
    grd = R.score(iou_min=MC.HAND_IOU, last_id=last, **x)
    for n, want in expect.items():
        assert np.array_equal(getattr(opt, n), want), n
    for n, want in greedy.items():
        assert np.array_equal(getattr(grd, n), want), n
    lane = {n: i for i, n in enumerate(MC.HAND)}
    assert (opt.tp[0, lane["cardinality"]], grd.tp[0, lane["cardinality"]]) == (2, 1)
    assert (grd.fn[0, lane["cardinality"]], grd.fp[0, lane["cardinality"]]) == (1, 1)
    iou = opt.iou[0, lane["cardinality"]]
    assert np.allclose(iou[:2, :2], [[15 / 25, 14 / 26], [14 / 26, 3 / 37]], atol=1e-12)
    s = lane["sum"]
    assert abs(grd.match_iou[0, s].sum() - (19 / 21 + 15 / 25)) < 1e-12 and abs(opt.match_iou[0, s].sum() - 2 * 18 / 22) < 1e-12
    assert opt.tp[0, lane["keep_wins"]] == 1 and opt.truth_match[0, lane["keep_wins"], 0] == 0      # kept although it costs a pair
    assert opt.tp[0, lane["nan_box"]] == 1 and opt.fp[0, lane["nan_box"]] == 1
    # every optimum of the hand cases is unique: brute force finds no other assignment of the same value
    for b in range(len(MC.HAND)):
        ok = M._ok(opt.iou[0, b], x["truth_present"][0, b], x["presence"][0, b], MC.HAND_IOU)
        kept, claimed = M.keep_step(ok, R.words(x["obj_id"])[0, b], last[b])
        w = M.weights(opt.iou[0, b], ok, kept, claimed)
        value, pairs = M.solve(w)
        for g, j in pairs:      # (forbidding any pair of the optimum lowers the value)
            v = w.copy()
            v[g, j] = -1
            assert M.solve_brute(v) < value


def _scored(x):
    return (np.asarray(x["truth_valid"]) != 0) & (np.asarray(x["map_count"]) != -1)


@pytest.mark.parametrize("i", range(len(MC.CASES)), ids=IDS)
def test_the_cases_tell_the_modes_apart_and_leave_few_lanes_out(i):
    c = MC.CASES[i]
    x = MC.make(c)
    on = _scored(x)
    grd, opt = R.score(iou_min=c.iou_min, **x), M.score(iou_min=c.iou_min, **x)
    differ = ((grd.truth_match != opt.truth_match).any(-1) & on).sum() / on.sum()
    differ_tp = ((grd.tp != opt.tp) & on).sum() / on.sum()
    differ_sum = ((np.abs(grd.match_iou.sum(-1) - opt.match_iou.sum(-1)) > 1e-9) & on).sum() / on.sum()
    first = M.fragile_from(opt.iou, x["truth_present"], x["presence"], on, c.iou_min)
    left_out = int((first < MC.T).sum())
    e = R.iou32_error(x["truth_box"], x["box"]) * M.UNIT
    tot = lambda s: dict(zip(R.COUNTS, s.counts.sum(0).tolist()))
    print(MC.case_id(c), "scored frames", int(on.sum()), "greedy and optimal differ in {:.3f} (tp {:.3f}, sum of IoU {:.3f})".format(
        differ, differ_tp, differ_sum), "left out", left_out, "e = {:.3f} x 2^-20".format(e), "tp", tot(grd)["tp"], "->", tot(opt)["tp"])
    M.record("cases", MC.case_id(c), scored_frames=int(on.sum()), differ=float(differ), differ_tp=float(differ_tp),
           differ_iou_sum=float(differ_sum), left_out=left_out, lanes=MC.B, e_units_of_2_pow_minus_20=float(e), greedy=tot(grd),
           optimal=tot(opt))
    assert left_out <= MC.FRAGILE_CAP * MC.B
    assert 0.0 < e < 4.0                       # (an fp32 IoU is good to a few 2^-24: well under four units of 2^-20)
    if c.G >= 2 and c.N >= 2:
        assert differ >= 0.1
        assert tot(opt)["tp"] > tot(grd)["tp"]
    else:
        assert differ == 0.0                   # one truth, one object: nothing to choose
    # the structure of the inputs: the non-finite lane, the lane without a valid frame, holes on the lane's side in the odd lanes
    assert (x["map_count"][MC.NAN_FROM:, MC.NAN_LANE] == -1).all() and not x["truth_valid"][:, MC.INVALID_LANE].any()
    assert opt.counts[MC.NAN_LANE, 1] == MC.T - MC.NAN_FROM and not opt.counts[MC.INVALID_LANE].any()
    if c.N >= 2:
        assert ((x["presence"][:, 1::2, :-1] == 0) & (x["presence"][:, 1::2, 1:] != 0)).any()


@pytest.mark.parametrize("i", [4, 9], ids=[IDS[4], IDS[9]])
def test_a_judge_accepts_the_optimum_and_rejects_what_is_not(i):
    c = MC.CASES[i]
    x = MC.make(c)
    opt = M.score(iou_min=c.iou_min, **x)
    frames = M.scored_frames(x)
    # the reference's own matching, imposed: clean, and the run it drives is the reference's
    judge = M.Judge([((t, b), opt.truth_match[t, b]) for t, b in frames], M.slack(1.0))
    with M.replaced(R, "assign", judge.assign):
        again = R.score(iou_min=c.iou_min, **x)
    assert judge.clean() and judge.asked == judge.judged == len(frames) and judge.worst_deficit == 0
    assert all(np.array_equal(a, b) for a, b in zip(again, opt))
    # the greedy matching, imposed: feasible, but short of the optimum in cardinality or sum in the frames where the modes differ
    grd = R.score(iou_min=c.iou_min, **x)
    judge = M.Judge([((t, b), grd.truth_match[t, b]) for t, b in frames], M.slack(1.0))
    with M.replaced(R, "assign", judge.assign):
        R.score(iou_min=c.iou_min, **x)
    assert not judge.infeasible and (judge.cardinality or judge.deficit)
    # a matching that gives an ineligible pair is infeasible
    bad = opt.truth_match.copy()
    t, b = next((t, b) for t, b in frames if (opt.truth_match[t, b] < 0).any() and x["truth_present"][t, b].all())
    bad[t, b] = 0
    judge = M.Judge([((t2, b2), bad[t2, b2]) for t2, b2 in frames], M.slack(1.0))
    with M.replaced(R, "assign", judge.assign):
        R.score(iou_min=c.iou_min, **x)
    assert (t, b) in judge.infeasible


def test_the_identity_and_the_link_take_the_same_assignment():
    c = MC.CASES[4]
    y = MC.identity_inputs(c)
    kw = dict(iou_min=0.3, reid_dist=4.0, reid_what=float("inf"), M=8, max_age=3)
    grd, opt = I.identity(**y, **kw), M.identity(**y, **kw)
    linked = lambda r: int(r.mem["counts"][:, 3:5].sum())        # kept + bridged: the position link's pairs
    print("identity: position links greedy", linked(grd), "optimal", linked(opt))
    assert linked(opt) > linked(grd)
    assert I._link is not M.link                                  # (the reference is as it was after the block)
    tab, tr, keep = MC.traj_inputs(c)
    g, o = TR.score(tab, tr, c.iou_min, keep), M.traj_score(tab, tr, c.iou_min, keep)
    print("trajectory link: linked greedy", int(g.lane_counts[:, 3].sum()), "optimal", int(o.lane_counts[:, 3].sum()))
    assert o.lane_counts[:, 3].sum() > g.lane_counts[:, 3].sum() and np.array_equal(o.lane_counts[:, :3], g.lane_counts[:, :3])
