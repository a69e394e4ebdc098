"""No GPU: the reference of track log stitching (tests/tracklog_stitch_ref.py) on the cases of tests/tracklog_stitch_cases.py, and
that each case exercises what it is there for.  The stitched table of a relabelled log is ``tracklog_ref.smooth`` of the log never
relabelled, array for array; a candidate's d2 is the Mahalanobis distance of densely assembled covariances (numpy.linalg); no case
leaves a decision to fp32 (``undecided`` == 0: asserted here, never skipped); the assignment is brute force's on the small tables."""
import numpy as np
import pytest

from sqair_amd import _capi
from tests import tracklog_ref as R
from tests import tracklog_score_ref as SCR
from tests import tracklog_stitch_cases as SC
from tests import tracklog_stitch_ref as SR

assert hasattr(_capi, "SqairTrackLogStitch")   # (the feature's ABI: nothing here passes without it)

TABLE = ("track_id", "n_tracks", "len0", "frame_index", "state", "size", "filt", "smooth", "filt32", "smooth32")
K = {n: i for i, n in enumerate(SCR.COUNTS)}
FILLED = SCR.VIEWS.index("smooth_filled")


@pytest.mark.parametrize("name", SC.NAMES)
def test_no_case_leaves_a_decision_to_fp32(name):
    assert SC.reference(name).stitch.undecided == 0


@pytest.mark.parametrize("name", SC.BITS + ("invalid_inside", "empty", "dropout"))
def test_the_stitched_table_is_the_solve_of_the_log_never_relabelled(name):
    ref = SC.reference(name)
    for k in TABLE:
        assert np.array_equal(getattr(ref.stitch.table, k), getattr(ref.plain, k)), (name, k)
    assert int(ref.stitch.n_links.sum()) > 0 and np.array_equal(ref.stitch.table.n_tracks, ref.solve.n_tracks - ref.stitch.n_links)


@pytest.mark.parametrize("name", [n for n in SC.NAMES if n != "limit"])
def test_d2_is_the_mahalanobis_distance_of_dense_covariances(name):
    c, ref = SC.make(name), SC.reference(name)
    f0f1 = [SR.spans(ref.solve.state, b) for b in range(ref.solve.track_id.shape[0])]
    n = 0
    for b, cands in enumerate(ref.stitch.cands):
        f0, f1 = f0f1[b]
        for k in cands:
            if not np.isfinite(k.d2):
                continue
            dense = SR.dense_d2(ref.solve.filt[f1[k.a], b, k.a], ref.solve.smooth[f0[k.c], b, k.c], k.steps, SC.Q)
            assert abs(k.d2 - dense) <= 1e-9 * abs(dense), (name, b, k, dense)
            assert k.steps == k.gap + 1 and k.gap <= c.max_gap
            n += 1
    assert n > 0 or name in ("nonfinite",)


@pytest.mark.parametrize("name", [n for n in SC.NAMES if n != "limit"])
def test_the_assignment_is_brute_forces(name):
    c, ref = SC.make(name), SC.reference(name)
    gate2 = float(np.float32(c.gate) * np.float32(c.gate))
    for b, cands in enumerate(ref.stitch.cands):
        w = SR.weight_table(cands, c.C, gate2)
        best, pairs = SR.solve(w)
        top, runner_up = SR.second_brute(w)
        assert best == top and (not pairs or SR.second(w, pairs) == runner_up), (name, b)
        assert {a: int(n) for a, n in enumerate(ref.stitch.link_next[b]) if n >= 0} == pairs


def test_relabel_and_chain_link_what_they_should():
    s = SC.reference("relabel").stitch
    assert s.link_next.tolist() == [[1, -1, -1, -1], [2, -1, -1, -1], [2, 3, -1, -1]] and s.n_links.tolist() == [1, 1, 2]
    assert s.link_gap.tolist() == [[4, -1, -1, -1], [4, -1, -1, -1], [4, 4, -1, -1]]
    assert s.root.tolist() == [[0, 0, -1, -1], [0, 1, 0, -1], [0, 1, 0, 1]]
    assert (SC.reference("relabel").solve.len0[0, :2] == 1).all()                       # track_len restarted at 1
    s = SC.reference("relabel_chain").stitch
    assert s.n_links.tolist() == [2, 2, 2] and s.root[0].tolist() == [0, 0, 0, -1] and s.root[2].tolist() == [0, 1, 0, 0]
    assert 0 in s.link_gap[0].tolist() and 0 in s.link_gap[1].tolist() and 0 in s.link_gap[2].tolist()    # a switch between consecutive frames
    assert (s.link_d2[s.link_next >= 0] > 0).all() and (s.link_d2[s.link_next < 0] == 0).all()


def test_crossing_position_alone_swaps_them_and_the_state_distance_does_not():
    c, ref = SC.make("crossing"), SC.reference("crossing")
    for b in range(3):
        f0, f1 = SR.spans(ref.solve.state, b)
        last = np.array([ref.solve.filt[f1[a], b, a, :, 0] for a in (0, 1)])            # the predecessors' last filtered centres
        born = np.array([ref.solve.smooth[f0[k], b, k, :, 0] for k in (2, 3)])          # the newborns' first centres
        dist = np.linalg.norm(last[:, None] - born[None], axis=-1)
        assert dist[0, 1] + dist[1, 0] < dist[0, 0] + dist[1, 1] and dist[0].argmin() == 1 and dist[1].argmin() == 0   # position alone: swapped
        assert ref.stitch.link_next[b].tolist() == [2, 3, -1, -1]
        d2 = {(k.a, k.c): k.d2 for k in ref.stitch.cands[b]}
        assert d2[0, 2] + d2[1, 3] < 1.0 < d2[0, 3] + d2[1, 2]


def test_refused_links_refuse_for_the_four_reasons():
    c, ref = SC.make("refused_links"), SC.reference("refused_links")
    assert int(ref.stitch.n_links.sum()) == 0 and (ref.stitch.link_next == -1).all() and (ref.stitch.link_gap == -1).all()
    assert (ref.stitch.link_d2 == 0).all() and ref.stitch.root[:, :2].tolist() == [[0, 1]] * 4
    (far,), none = ref.stitch.cands[0], ref.stitch.cands[1:]
    assert far.d2 > c.gate ** 2 and not far.eligible and [len(k) for k in none] == [0, 0, 0]
    pre = lambda b: np.concatenate([[0], np.cumsum(R.window(c.log, b, c.lag)[2])])
    sp = [SR.spans(ref.solve.state, b) for b in range(4)]
    assert pre(1)[sp[1][0][1]] - pre(1)[sp[1][1][0] + 1] == 5 > c.max_gap               # the gap
    assert ref.solve.len0[2].tolist()[:2] == [1, 4]                                     # the successor is older than its first frame here
    assert sp[3][1][0] >= sp[3][0][1]                                                   # the spans overlap
    for k in ("state", "size", "filt", "smooth", "track_id", "len0", "n_tracks"):
        assert np.array_equal(getattr(ref.stitch.table, k), getattr(ref.solve, k)), k   # nothing linked: the solve's table


def test_invalid_frames_inside_the_gap_do_not_count_and_are_state_3():
    c, ref = SC.make("invalid_inside"), SC.reference("invalid_inside")
    assert ref.stitch.link_gap[:, 0].tolist() == [3, 3, 3] and ref.stitch.n_links.tolist() == [1, 1, 1]        # five frames, two invalid
    st = ref.stitch.table.state
    assert st[10:15, 0, 0].tolist() == [2, 3, 3, 2, 2] and st[10:15, 1, 0].tolist() == [3, 2, 2, 2, 3]
    assert st[5, 2, 0] == 3 and st[10:15, 2, 0].tolist() == [2, 2, 3, 3, 2]
    assert all(k.steps == 4 for cands in ref.stitch.cands for k in cands)


def test_young_wrapped_dropped_nonfinite_and_empty_hold_what_they_say():
    c, ref = SC.make("young_and_wrapped"), SC.reference("young_and_wrapped")
    assert c.log["count"].tolist() == [15, 40, 24] and (ref.solve.frame_index[:9, 0] == -1).all() and c.log["count"][1] > c.L
    assert ref.solve.len0[1, 0] > 1 and ref.stitch.link_next[:, 0].tolist() == [1, 1, 1]                       # an old predecessor may link
    c, ref = SC.make("dropped_root"), SC.reference("dropped_root")
    assert ref.solve.n_tracks.tolist() == [6, 5, 2] and ref.solve.track_id[0].tolist() == [2, 3, 4, 5]
    assert ref.stitch.link_next[0].tolist() == [1, 2, 3, -1] and ref.stitch.table.track_id[0].tolist() == [2, -1, -1, -1]
    assert ref.stitch.table.n_tracks.tolist() == [3, 3, 1] and ref.stitch.table.len0[0, 0] == 1
    assert ref.stitch.link_next[1].tolist() == [1, 3, -1, -1] and ref.stitch.table.track_id[1].tolist() == [1, 3, -1, -1]
    assert ref.stitch.root[1].tolist() == [0, 0, 1, 0]                                                          # id 3's predecessor (id 0) is not kept
    c, ref = SC.make("nonfinite"), SC.reference("nonfinite")
    assert ref.stitch.n_links.tolist() == [0, 1, 0] and np.isnan(ref.solve.filt[9, 0, 0, 0, 0])
    assert np.isfinite(ref.stitch.link_d2).all() and (ref.stitch.link_d2[[0, 2]] == 0).all()
    c, ref = SC.make("empty"), SC.reference("empty")
    assert ref.solve.n_tracks.tolist() == [2, 0, 2] and (ref.stitch.root[1] == -1).all() and (ref.stitch.table.state[:, 1] == 0).all()


def test_limit_runs_the_assignment_at_its_limits():
    c, ref = SC.make("limit"), SC.reference("limit")
    assert (c.C, c.N, c.L, c.lag) == (64, 16, 64, 64) and (ref.solve.track_id >= 0).all()
    assert ref.stitch.n_links.tolist() == [32, 32] and ref.stitch.table.n_tracks.tolist() == [32, 32]
    assert all(len(cands) > 64 for cands in ref.stitch.cands)
    for b in range(2):
        assert sorted(ref.stitch.root[b].tolist()) == sorted(list(range(32)) * 2)


def test_dropout_scored_before_and_after_stitching():
    """smooth_filled before: idsw 1, IDF1 1/3, gap_tp 0 (12 of 24 truths tracked under two ids, the gap a hole); after: idsw 0, IDF1 1,
    gap_tp 12 -- recorded as they come out of tests/tracklog_score_ref.py."""
    c, ref = SC.make("dropout"), SC.reference("dropout")
    assert sorted(set(c.log["log_id"][c.log["log_id"] >= 0].tolist())) == [0, 1] and ref.stitch.link_gap[0, 0] == 12
    before = SCR.score(SC.table_of(ref.solve), c.log["log_valid"], c.truth, SC.IOU_MIN)
    after = SCR.score(SC.table_of(ref.stitch.table), c.log["log_valid"], c.truth, SC.IOU_MIN)
    fig = lambda s: {n: (SCR.pooled(s.counts, s.sums, FILLED)[n] if n == "idf1" else int(s.counts[:, FILLED, K[n]].sum()))
                     for n in ("idsw", "idf1", "gap_tp", "tp", "fn")}
    print("dropout, smooth_filled: before", fig(before), "after", fig(after))
    assert fig(after)["idsw"] == 0 and fig(after)["idf1"] == 1.0 and fig(after)["gap_tp"] == 12 and fig(after)["fn"] == 0
    assert fig(before) == dict(idsw=1, idf1=1.0 / 3.0, gap_tp=0, tp=12, fn=12)
