"""No GPU: the float64 reference of lane identities (tests/identity_ref.py) held to answers known by hand -- a best-row switch, a
drop-out bridged by re-identification, the same drop-out after max_age, appearance against distance, the eviction order, the tie
rules, a non-finite frame, a reset -- and the inputs of the kernel test (tests/identity_cases.py) held to the cap on fragile lanes
from the reference alone: the fp32 restatement of the three compared quantities (IoU, dc2, dw) is measured against float64 on those
very inputs, and a lane is fragile from its first frame on which a decisive compare lies within four times that error."""
import numpy as np
import pytest

from tests import identity_cases as IC
from tests import identity_ref as IR
from tests import score_ref as SR

NW = 3
INF = float("inf")


def _lane(frames, N, nw=NW):
    """One lane from ``frames``: per frame None (a non-finite frame) or a list of N slots, each None (absent) or (box, id, what)."""
    T = len(frames)
    x = dict(box=np.zeros((T, 1, N, 4), np.float32), presence=np.zeros((T, 1, N), np.float32), obj_id=np.zeros((T, 1, N), np.float32),
             what=np.zeros((T, 1, N, nw), np.float32), best_row=np.zeros((T, 1), np.int32))
    for t, f in enumerate(frames):
        if f is None:
            x["best_row"][t, 0] = -1
            continue
        for j, s in enumerate(f):
            if s is not None:
                x["box"][t, 0, j], x["presence"][t, 0, j], x["obj_id"][t, 0, j], x["what"][t, 0, j] = s[0], 1.0, s[1], s[2]
    return x


def _run(frames, N=2, M=4, iou_min=0.3, reid_dist=4.0, reid_what=INF, max_age=3, nw=NW, **kw):
    return IR.identity(iou_min=iou_min, reid_dist=reid_dist, reid_what=reid_what, M=M, max_age=max_age, **dict(_lane(frames, N, nw), **kw))


def _counts(r):
    return dict(zip(IR.COUNTS, r.mem["counts"][0].tolist()))


A, Bq = np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0])
BOX = (10.0, 10.0, 12.0, 12.0)


def _at(dy, dx=0.0):
    return (BOX[0] + dy, BOX[1] + dx, BOX[2], BOX[3])


def test_a_word_switch_keeps_the_lane_id_and_counts_no_identity_switch():
    """The obj_id word changes at frame 3 while the box does not move: lane_id stays, how = 2 (bridged), and the score's reference
    counts one identity switch on obj_id and none on lane_id."""
    frames = [[(_at(0.5 * t), 5.0 if t < 3 else 9.0, A), None] for t in range(6)]
    r = _run(frames)
    assert r.lane_id[:, 0, 0].tolist() == [0] * 6 and (r.lane_id[:, 0, 1] == -1).all()
    assert r.how[:, 0, 0].tolist() == [0, 1, 1, 2, 1, 1] and r.track_len[:, 0, 0].tolist() == [1, 2, 3, 4, 5, 6]
    assert _counts(r) == dict(frames=6, frames_invalid=0, objects=6, kept=4, bridged=1, reidentified=0, born=1, ended=0)
    x = _lane(frames, 2)
    truth = dict(truth_box=x["box"][:, :, :1].copy(), truth_present=np.ones((6, 1, 1), np.int32), truth_valid=np.ones((6, 1), np.int32))
    args = dict(box=x["box"], presence=x["presence"], map_count=np.ones((6, 1), np.int32), iou_min=0.5, **truth)
    on_rows = SR.score(obj_id=x["obj_id"], **args)
    on_lanes = SR.score(obj_id=r.lane_id.view(np.float32), **args)      # (the score takes the id as a 32-bit word)
    assert on_rows.counts[0, SR.COUNTS.index("idsw")] == 1 and on_lanes.counts[0, SR.COUNTS.index("idsw")] == 0
    assert on_rows.counts[0, SR.COUNTS.index("tp")] == on_lanes.counts[0, SR.COUNTS.index("tp")] == 6


def test_a_return_inside_the_reid_gate_keeps_the_id_and_after_max_age_it_does_not():
    """Seen at frame 0, unseen for three frames (age 3 = max_age: still remembered), back at frame 4 displaced by 14 px: the IoU is 0,
    the centre moved 14 <= 4 * (3 + 1) = 16 -> the same id, how = 3.  One frame more unseen and the track has ended: a new id."""
    seen, away = [(BOX, 5.0, A), None], [None, None]
    back = [(_at(14.0), 8.0, A), None]
    r = _run([seen, away, away, away, back])
    assert r.lane_id[[0, 4], 0, 0].tolist() == [0, 0] and r.how[4, 0, 0] == IR.REID and r.track_len[4, 0, 0] == 2
    assert _counts(r) == dict(frames=5, frames_invalid=0, objects=2, kept=0, bridged=0, reidentified=1, born=1, ended=0)
    assert r.mem["trk_age"][0, 0] == 0 and r.mem["trk_word"][0, 0] == np.float32(8.0).view(np.int32) and r.mem["next_id"][0] == 1
    assert np.array_equal(r.mem["trk_box"][0, 0], np.float32(_at(14.0)))
    r = _run([seen, away, away, away, away, back])
    assert r.lane_id[[0, 5], 0, 0].tolist() == [0, 1] and r.how[5, 0, 0] == IR.BORN and r.track_len[5, 0, 0] == 1
    assert _counts(r) == dict(frames=6, frames_invalid=0, objects=2, kept=0, bridged=0, reidentified=0, born=2, ended=1)
    # just outside the gate: 17 px > 16
    r = _run([seen, away, away, away, [(_at(17.0), 8.0, A), None]])
    assert r.lane_id[4, 0, 0] == 1 and r.how[4, 0, 0] == IR.BORN
    # re-identification off: born
    r = _run([seen, away, away, away, back], reid_dist=0.0)
    assert r.lane_id[4, 0, 0] == 1 and r.how[4, 0, 0] == IR.BORN


def test_appearance_picks_the_farther_of_two_unseen_tracks_and_distance_the_nearer():
    two = [(_at(0.0, 0.0), 1.0, A), (_at(0.0, 20.0), 2.0, Bq)]      # track 0 looks like A, track 1 like B
    away = [None, None]
    back = [(_at(0.0, 7.0), 9.0, Bq), None]                          # 7 px from track 0, 13 px from track 1, looks like B
    r = _run([two, away, back], iou_min=0.9)                         # (r = 4 * 2 = 8 would gate track 1: a wider gate below)
    assert r.lane_id[2, 0, 0] == 0 and r.how[2, 0, 0] == IR.REID    # only track 0 is inside the gate
    r = _run([two, away, back], iou_min=0.9, reid_dist=8.0)
    assert r.lane_id[2, 0, 0] == 1 and r.how[2, 0, 0] == IR.REID    # both inside: the appearance decides
    r = _run([two, away, back], iou_min=0.9, reid_dist=8.0, reid_what=0.1)
    assert r.lane_id[2, 0, 0] == 1                                   # dw(B, B) = 0 <= 0.1; track 0 (dw = 2 / 3) is gated
    r = _run([two, away, [(_at(0.0, 7.0), 9.0, 0.5 * (A + Bq)), None]], iou_min=0.9, reid_dist=8.0, reid_what=0.1)
    assert r.lane_id[2, 0, 0] == 2 and r.how[2, 0, 0] == IR.BORN    # dw = 1 / 6 to both: neither passes
    r = _run([two, away, back], iou_min=0.9, reid_dist=8.0, appearance=False)
    assert r.lane_id[2, 0, 0] == 0 and r.mem["trk_what"] is None    # without trk_what: the nearer one


def test_eviction_takes_the_oldest_unclaimed_entry_ties_to_the_smallest():
    far = lambda k: (40.0 * k, 200.0, 10.0, 10.0)
    obj = lambda k, i: (far(k), float(i), A)
    # M = 2 = N, max_age large, re-identification off: two tracks, both unseen (ages 1, 1), then two strangers
    r = _run([[obj(0, 1), obj(1, 2)], [None, None], [obj(2, 3), obj(3, 4)]], M=2, max_age=9, reid_dist=0.0)
    assert r.lane_id[2, 0].tolist() == [2, 3] and (r.how[2, 0] == IR.BORN).all()
    assert r.mem["trk_id"][0].tolist() == [2, 3] and _counts(r)["ended"] == 2      # entry 0 first (the tie), then entry 1
    # ages 2 and 1: the older entry (1) goes first although its index is larger
    r = _run([[obj(0, 1), obj(1, 2)], [obj(0, 1), None], [None, None], [obj(2, 3), None]], M=2, max_age=9, reid_dist=0.0)
    assert r.mem["trk_id"][0].tolist() == [0, 2] and r.lane_id[3, 0, 0] == 2 and _counts(r)["ended"] == 1
    assert r.mem["trk_age"][0].tolist() == [2, 0]
    # a matched entry is never evicted: the stranger takes the unclaimed one
    r = _run([[obj(0, 1), obj(1, 2)], [obj(0, 1), obj(2, 3)]], M=2, max_age=9, reid_dist=0.0)
    assert r.lane_id[1, 0].tolist() == [0, 2] and r.how[1, 0].tolist() == [IR.KEPT, IR.BORN] and r.mem["trk_id"][0].tolist() == [0, 2]
    # the first free entry before any eviction
    r = _run([[obj(0, 1), None], [None, obj(1, 2)]], M=3, max_age=9, reid_dist=0.0)
    assert r.mem["trk_id"][0].tolist() == [0, 1, -1] and r.mem["trk_age"][0, 0] == 1


def test_the_tie_rules():
    # two tracks with the very same box, one slot with those words: IoU 1 with both, the smallest entry wins the greedy scan ...
    same = [(BOX, 1.0, A), (BOX, 2.0, Bq)]
    r = _run([same, [(BOX, 7.0, A), None]])
    assert r.lane_id[1, 0, 0] == 0 and r.how[1, 0, 0] == IR.BRIDGED
    # ... unless the slot carries the other track's word: the same lineage first
    r = _run([same, [(BOX, 2.0, A), None]])
    assert r.lane_id[1, 0, 0] == 1 and r.how[1, 0, 0] == IR.KEPT
    # one track, two slots with its very box: the smallest slot; the other slot is born
    r = _run([[(BOX, 1.0, A), None], [(BOX, 5.0, A), (BOX, 6.0, A)]])
    assert r.lane_id[1, 0].tolist() == [0, 1] and r.how[1, 0].tolist() == [IR.BRIDGED, IR.BORN]
    # re-identification: two unseen tracks equally far and alike -> the smallest entry
    two = [(_at(0.0, -6.0), 1.0, A), (_at(0.0, 6.0), 2.0, A)]
    r = _run([two, [None, None], [(_at(0.0, 0.0), 9.0, A), None]], iou_min=0.9)
    assert r.lane_id[2, 0, 0] == 0 and r.how[2, 0, 0] == IR.REID
    # re-identification is greedy in j: slot 0 takes the track slot 1 would have matched better
    r = _run([[(BOX, 1.0, A), None], [None, None], [(_at(0.0, 5.0), 8.0, Bq), (_at(0.0, 7.5), 9.0, A)]], iou_min=0.9)
    assert r.lane_id[2, 0].tolist() == [0, 1] and r.how[2, 0].tolist() == [IR.REID, IR.BORN]
    # a NaN never passes: a NaN box is born, a NaN what is not re-identified
    nan_box = (np.nan, 10.0, 12.0, 12.0)
    r = _run([[(BOX, 1.0, A), None], [(nan_box, 1.0, A), None]])
    assert r.how[1, 0, 0] == IR.BORN and r.lane_id[1, 0, 0] == 1
    r = _run([[(BOX, 1.0, A), None], [None, None], [(_at(3.0), 1.0, A * np.nan), None]], iou_min=0.9)
    assert r.how[2, 0, 0] == IR.BORN


def test_a_non_finite_frame_leaves_the_memory_untouched():
    seen = [(BOX, 5.0, A), None]
    r = _run([seen, None, None, None, None, None, seen], max_age=1)
    assert (r.lane_id[1:6] == -1).all() and (r.how[1:6] == -1).all() and (r.track_len[1:6] == -1).all()
    assert r.lane_id[6, 0, 0] == 0 and r.how[6, 0, 0] == IR.KEPT and r.track_len[6, 0, 0] == 2      # no ageing in between
    assert _counts(r) == dict(frames=2, frames_invalid=5, objects=2, kept=1, bridged=0, reidentified=0, born=1, ended=0)


def test_a_reset_frees_the_entries_and_keeps_next_id_and_two_passes_equal_one():
    frames = [[(_at(0.5 * t), 5.0, A), (_at(0.5 * t, 20.0), 6.0, Bq)] for t in range(6)]
    x = _lane(frames, 2)
    kw = dict(iou_min=0.3, reid_dist=4.0, reid_what=INF, M=4, max_age=3)
    whole = IR.identity(**kw, **x)
    first = IR.identity(**kw, **{k: v[:3] for k, v in x.items()})
    second = IR.identity(mem=first.mem, **kw, **{k: v[3:] for k, v in x.items()})
    assert np.array_equal(np.concatenate([first.lane_id, second.lane_id]), whole.lane_id)
    assert all(np.array_equal(second.mem[k], whole.mem[k]) for k in IR.MEMORY)
    mem = dict(first.mem, trk_id=-np.ones_like(first.mem["trk_id"]))      # the caller's reset
    after = IR.identity(mem=mem, **kw, **{k: v[3:] for k, v in x.items()})
    assert after.lane_id[0, 0].tolist() == [2, 3] and (after.how[0, 0] == IR.BORN).all() and after.mem["next_id"][0] == 4
    assert after.track_len[0, 0].tolist() == [1, 1]


@pytest.mark.parametrize("i", range(len(IC.CASES)), ids=[IC.case_id(c) for c in IC.CASES])
def test_the_kernel_tests_inputs_stay_under_the_cap_on_fragile_lanes(i):
    c = IC.CASES[i]
    x = IC.make(c)
    tol = IR.measured_tol(x["box"], x["best_row"], x["what"], c.appearance)
    print(IC.case_id(c), "fp32 restatement against float64, times four:", tol)
    # the bands are small next to what they are compared with: iou_min = 0.3, r * r >= 16, what vectors that differ by O(1)
    assert 0 < tol.iou < 1e-5 and 0 < tol.dc2 < 1e-2 and tol.dw < 1e-4 and (tol.dw > 0) == c.appearance
    ref = IR.identity(iou_min=IC.IOU_MIN, reid_dist=c.reid_dist, reid_what=c.reid_what, M=c.M, max_age=IC.MAX_AGE, appearance=c.appearance,
                      tol=tol, **x)
    fragile = int((ref.fragile_from < IC.T).sum())
    tot = dict(zip(IR.COUNTS, ref.mem["counts"].sum(0).tolist()))
    print(IC.case_id(c), "fragile lanes:", fragile, "of", IC.B, tot)
    assert fragile <= IC.FRAGILE_CAP * IC.B
    need = ("kept", "bridged", "born", "ended") + (("reidentified",) if c.reid_dist > 0 else ())
    assert all(tot[n] > 0 for n in need), tot
    if c.M == c.N and c.N > 1:      # the full table: births that evict
        assert tot["ended"] > 0.3 * tot["born"]
    # drop-outs on both sides of max_age and returns on both sides of the gate are in the inputs: tracks end by age, objects come back
    assert tot["frames_invalid"] == IC.T - IC.NAN_FROM and tot["frames"] == IC.T * IC.B - tot["frames_invalid"]
