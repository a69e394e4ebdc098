"""No GPU: the float64 reference of lane motion (tests/motion_ref.py) on its own -- the inputs of tests/motion_cases.py hold the
fragility cap from the reference alone, every event and both kinds of movers occur, one axis seen every frame converges to the
closed-form steady-state gains of the alpha-beta filter, and the two hand-made scenarios give the figures the feature was specified
with: ids that break without the filter (tests/identity_ref.py on the same inputs) and hold with it."""
import numpy as np
import pytest

from tests import motion_cases as MC
from tests import motion_ref as MR

S = MC.SCALARS


@pytest.mark.parametrize("i", range(len(MC.CASES)), ids=[MC.case_id(c) for c in MC.CASES])
def test_the_cases_hold_the_fragile_cap_and_exercise_every_event(i):
    c = MC.CASES[i]
    x, ref, tol, first = MC.reference(i)
    whole = first == MC.T
    left_out = int((~whole).sum())
    tot = dict(zip(MR.COUNTS, ref.mem["counts"][whole].sum(0).tolist()))
    print(MC.case_id(c), "band", tol, "left out", left_out, tot, "bars", MR.bars(ref.err, whole))
    assert left_out <= MC.FRAGILE_CAP * MC.B
    assert all(0.0 < v < 1e-3 for v in (tol.iou, tol.d2)) and (tol.dw > 0.0) == c.appearance      # (a band, and a narrow one)
    assert all(tot[n] > 0 for n in ("kept", "bridged", "reidentified", "born", "ended")), tot
    assert tot["objects"] == tot["kept"] + tot["bridged"] + tot["reidentified"] + tot["born"]
    # fast movers are followed: linked slots whose track moves faster than the IoU gate could follow from the last box
    speed = np.abs(ref.velocity).max(-1)
    assert ((speed > 6.0) & (ref.how >= MR.KEPT))[:, whole].sum() > 20
    # the conventions of the non-finite and the empty lane
    assert (ref.lane_id[MC.NAN_FROM:, MC.NAN_LANE] == -1).all() and (ref.velocity[MC.NAN_FROM:, MC.NAN_LANE] == 0).all()
    assert ref.mem["counts"][MC.NAN_LANE, :2].tolist() == [MC.NAN_FROM, MC.T - MC.NAN_FROM]
    assert ref.mem["counts"][MC.EMPTY_LANE].tolist() == [MC.T] + [0] * 7
    # velocity and nis are 0 for absent slots and newborns
    quiet = (ref.how == MR.BORN) | (ref.how == -1)
    assert (ref.velocity[quiet] == 0).all() and (ref.nis[quiet] == 0).all()


@pytest.mark.parametrize("q, r", [(0.25, 1.0), (1.0, 4.0), (0.01, 2.0)])
def test_one_axis_converges_to_the_closed_form_gains(q, r):
    """An axis seen every frame: the covariance recursion has a fixed point, Kalata's alpha-beta filter for the tracking index
    sqrt(q / r).  The gains the reference applies in its update -- k0 = Ppp'/S, k1 = Ppv'/S -- converge to it."""
    s = MR.Scalars(q, r, 16.0, 3.0)
    k = np.zeros((1, 2, 5))
    k[0, :] = (0.0, 0.0, r, 0.0, 16.0)
    live = np.array([True])
    for t in range(200):
        S_ = MR.predict(k, live, s, np.float64)
        k0, k1 = k[0, 0, 2] / S_[0, 0], k[0, 0, 3] / S_[0, 0]
        for ax in range(2):
            MR.update(k[0, ax], S_[0, ax], 2.0 * t, np.float64)
    alpha, beta = MR.steady_state(q, r)
    assert abs(k0 - alpha) < 1e-9 and abs(k1 - beta) < 1e-9, (k0, alpha, k1, beta)
    assert abs(k[0, 0, 1] - 2.0) < 1e-9 and abs(k[0, 0, 0] - 2.0 * 199) < 1e-6      # (a steady mover is followed without lag)
    assert abs(k[0, 0, 2] - alpha * r) < 1e-9                                        # (the posterior variance of the position)


@pytest.mark.parametrize("step", [(8.0, 0.0), (6.0, 6.0)], ids=["along_y", "diagonal"])
def test_the_fast_mover(step):
    """A 10 x 10 box moving 8 px a frame (or (6, 6)): IoU with its own last box 0.111 (0.087), centre distance 8 (8.49) > reid_dist =
    4 -- a fresh id every frame without the filter; with it frame 1 links through the gate (how = 3) and the rest by position."""
    x = MC.fast_mover(step)
    plain = MR.scenario_plain(x, 4.0, 10)
    assert plain.lane_id.ravel().tolist() == [0, 1, 2, 3, 4, 5] and (plain.how == MR.BORN).all()
    ref = MR.scenario_run(x, 4.0, 10, S)
    assert ref.lane_id.ravel().tolist() == [0] * 6 and ref.how.ravel().tolist() == [0, 3, 1, 1, 1, 1]
    assert ref.track_len.ravel().tolist() == [1, 2, 3, 4, 5, 6]
    piou = [MR.predicted_iou(x, t, 4.0, 10, S) for t in range(1, 6)]
    print(step, "velocity", ref.velocity[:, 0, 0].round(3).tolist(), "nis", ref.nis.ravel().round(3).tolist(), "predicted IoU", np.round(piou, 3))
    assert piou[0] < 0.3 and all(p >= 0.3 for p in piou[1:]) and piou == sorted(piou)
    if step == (8.0, 0.0):
        assert all(p >= 0.9 for p in piou[2:])
        assert np.allclose(ref.velocity[1:4, 0, 0, 0], [7.14, 7.80, 7.96], atol=0.005) and (ref.velocity[..., 1] == 0).all()
        assert abs(ref.nis[1, 0, 0] - 3.54) < 0.005 and abs(piou[1] - 0.77) < 0.005
    assert abs(ref.velocity[5, 0, 0, 0] - step[0]) < 0.03 and ref.nis[1, 0, 0] <= 9.0


def test_the_moving_drop_out():
    """3 px a frame, seen in frames 0-4 and 9-10: it returns 15 px from where it was last seen -- IoU 0, and outside reid_dist *
    (age + 1) = 10 -- and is born again without the filter; with it the track coasts, trk_age counts 4, the coasted box at frame 8 is
    within 0.1 px of the true one, and the predicted box at frame 9 overlaps the object's by 0.999: the position link keeps the id."""
    x, true = MC.moving_dropout()
    plain = MR.scenario_plain(x, 2.0, 10)
    assert plain.lane_id.ravel()[[4, 9, 10]].tolist() == [0, 1, 1] and plain.how[9, 0, 0] == MR.BORN
    ref = MR.scenario_run(x, 2.0, 10, S)
    assert ref.lane_id.ravel().tolist() == [0] * 5 + [-1] * 4 + [0, 0]
    assert ref.how.ravel().tolist() == [0, 1, 1, 1, 1, -1, -1, -1, -1, 1, 1]
    assert ref.track_len.ravel()[[4, 9, 10]].tolist() == [5, 6, 7]
    at8 = MR.scenario_run(x, 2.0, 10, S, frames=9).mem
    assert at8["trk_age"][0, 0] == 4 and at8["trk_id"][0, 0] == 0
    assert np.abs(at8["trk_kf"][0, 0, :, 0] - true[8]).max() < 0.1                   # (the box is 10 x 10: the centre says it)
    assert abs(MR.predicted_iou(x, 9, 2.0, 10, S) - 0.999) < 0.0005
    # the velocity along y: 2.98 in the fourth frame it is seen in (frame 3), 3.00 in frame 4
    print("velocity", ref.velocity[:, 0, 0, 0].round(3).tolist())
    assert abs(ref.velocity[3, 0, 0, 0] - 2.98) < 0.005 and abs(ref.velocity[4, 0, 0, 0] - 3.0) < 0.005


def test_the_noisy_moving_drop_out():
    """The same with sigma = 0.5 px of measurement noise (fixed seed): the predicted box at frame 9 overlaps by 0.61, still a link."""
    x, _ = MC.moving_dropout(0.5)
    assert MR.scenario_plain(x, 2.0, 10).lane_id.ravel()[[4, 9, 10]].tolist() == [0, 1, 1]
    ref = MR.scenario_run(x, 2.0, 10, S)
    assert ref.lane_id.ravel()[[4, 9, 10]].tolist() == [0, 0, 0] and ref.how.ravel()[[9, 10]].tolist() == [1, 1]
    assert abs(MR.predicted_iou(x, 9, 2.0, 10, S) - 0.61) < 0.005
