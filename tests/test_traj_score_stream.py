"""-m gpu: trajectory scoring from the stream (SqairStream.forecast / tracks(lane=True, truth=...), trajectory_score; include/sqair_hip.h:
sqair_lane_traj_score): B = 4, K = 5, N = 3, one frame per step, history = 8, SMC, eight steps, then forecasts of F = 4 frames with
S = 4 samples and traces of lag = 6.

A tracker with random parameters does not follow the generator's truth, so -- as tests/test_score_stream.py does -- the truth is made
from an untruthed call's own lane table: its boxes jittered, rotated into G = 4 truth slots, some anchors dropped (unlinked lane
objects), some truths ended early (gone), a stranger in the spare slot (an unlinked truth), present wherever the table holds no
living object (lost).  Checked here: the score equals the float64 reference (tests/traj_score_ref.py) applied to the returned table --
integers exactly, floats within four times the measured error of the fp32 restatement on those inputs, no lane fragile (asserted);
every other output of ``forecast`` / ``tracks`` is bit-identical to the call without ``truth``; with the truth equal to the table's own
``box0`` / ``box_mean`` every pair has IoU exactly 1 and error 0 and hits == pairs; ``trajectory_score()`` after two calls and after
``reset=True``; ``tracks`` and ``forecast`` between the same two steps give the same ``link``; ``link_ids=True`` on a scored stream."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import traj_score_ref as R
from tests.stream_harness import OUTS, host, same_bits, setup, stream

pytestmark = pytest.mark.gpu

HW = (50, 50)
B, K, N, G = 4, 5, 3, 4
STEPS, FH, S, LAG = 8, 4, 4, 6
IOU = 0.5


@pytest.fixture(scope="module")
def stepped():
    """A scored SMC stream with a history after eight steps (its steps scored against a truth made from an unscored run of the same
    seeds, so that the identity memory is filled), and the last step's truth."""
    F, P, obs, noise = setup(dict(k_particles=K, n_steps_per_image=N), B, STEPS, HW)
    kw = dict(outputs=OUTS, estimate=True, estimate_iou=IOU, resample="systematic", ess_frac=0.5, seed=5, history=8)
    first = stream((F, HW, P), B, **kw)
    rng = np.random.default_rng(7)
    truths = []
    for t in range(STEPS):
        lane = host(first.step(obs[t:t + 1], noise=noise[t:t + 1]))["lane"]
        box, present = np.zeros((1, B, G, 4), np.float32), np.zeros((1, B, G), np.int32)
        for j in range(N):
            box[0, :, j + 1] = lane["box"][0, :, j] + rng.standard_normal((B, 4))
            present[0, :, j + 1] = lane["presence"][0, :, j] != 0
        truths.append(dict(box=box, present=present))
    first.close()
    st = stream((F, HW, P), B, score=True, score_iou=IOU, score_truth=G, **kw)
    for t in range(STEPS):
        st.step(obs[t:t + 1], noise=noise[t:t + 1], truth=truths[t])
    yield st, truths[-1]
    st.close()


def _table(lane):
    return {n: lane[n] for n in _capi.TRAJ_TABLE_FIELDS if n in lane}


def _make_truth(lane, F, seed, tracks):
    """A ``truth`` dict from a lane table (host arrays): see the module's docstring."""
    rng = np.random.default_rng(seed)
    pres = lane["presence"] != 0                                        # [B, N]
    a_box, a_present = np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32)
    box, present = np.zeros((F, B, G, 4), np.float32), np.zeros((F, B, G), np.int32)
    for j in range(N):
        g = j + 1                                                       # rotated: object j is truth slot j + 1, slot 0 is spare
        a_box[:, g] = lane["box0"][:, j] + 0.75 * rng.standard_normal((B, 4))
        a_present[:, g] = pres[:, j] & (rng.uniform(size=B) < 0.85)     # a dropped anchor: an unlinked lane object
        mean = np.where(np.isfinite(lane["box_mean"][:, :, j]), lane["box_mean"][:, :, j], lane["box0"][None, :, j])
        box[:, :, g] = mean + 1.5 * rng.standard_normal((F, B, 4))
        end = np.where(rng.uniform(size=B) < 0.4, rng.integers(1, F + 1, B), F)
        live = np.arange(F)[:, None] < end[None] if not tracks else np.arange(F)[:, None] >= (F - end)[None]
        present[:, :, g] = a_present[None, :, g] & live                 # ended early (a forecast) or born late (a trace): gone
    stranger = rng.uniform(size=B) < 0.5                                # a truth nobody holds: unlinked
    a_box[stranger, 0], a_present[stranger, 0] = (2.0, 30.0, 9.0, 9.0), 1
    box[:, stranger, 0], present[:, stranger, 0] = (2.0, 30.0, 9.0, 9.0), 1
    valid = (rng.uniform(size=(F, B)) < 0.9).astype(np.int32)
    t = dict(box=box, present=present, valid=valid, anchor_box=a_box, anchor_present=a_present)
    if tracks:                                                          # a trace's anchor IS its newest frame
        box[F - 1], present[F - 1], valid[F - 1] = a_box, a_present, 1
    return t


def _reference(lane, truth, keep=None, acc=None):
    tr = dict(anchor_box=truth["anchor_box"], anchor_present=truth["anchor_present"],
              anchor_valid=truth.get("anchor_valid", np.ones(B, np.int32)), truth_box=truth["box"], truth_present=truth["present"],
              truth_valid=truth.get("valid", np.ones(truth["present"].shape[:2], np.int32)))
    tab = _table(lane)
    acc = acc or {}
    ref = R.score(tab, tr, IOU, keep, counts=acc.get("counts"), sums=acc.get("sums"), lane_counts=acc.get("lane_counts"))
    bar = R.bars(R.fp32_errors(tab, tr, ref))
    assert not R.fragile_lanes(tab, tr, ref, IOU, max(bar["link_iou"], bar["pair_iou"], 1e-6)).any(), "a decision within the bar"
    return ref, bar


def _check(score, ref, bar):
    assert set(score) == set(_capi.TRAJ_FIELDS)
    for n in R.INT_OUT:
        assert score[n].dtype == np.int32 and np.array_equal(score[n], getattr(ref, n)), (n, score[n], getattr(ref, n))
    # (the bars are measured; these caps only say that a bar is a rounding error: a ratio in [0, 1] carries a few 2^-24, a centre --
    # a coordinate of up to 64 px, spaced 2^-18 in fp32 -- up to two spacings, and the bar is four times that)
    cap = dict(link_iou=1e-5, p_alive=1e-5, pair_iou=1e-5, centre_err=4 * 2 * 2.0 ** -18)
    for n in R.FLOAT_OUT:
        err = float(np.abs(score[n].astype(np.float64) - getattr(ref, n)).max())
        assert bar[n] < cap[n] and err <= bar[n], (n, err, bar[n])


def _check_accumulated(got, ref, bar, calls):
    for i, n in enumerate(R.COUNTS):
        assert got[n].dtype == torch.int64 and np.array_equal(got[n].numpy(), ref.counts[..., i]), n
    for i, n in enumerate(R.LANE_COUNTS):
        assert np.array_equal(got[n].numpy(), ref.lane_counts[:, i]), n
    terms = (ref.counts[..., 1], ref.counts[..., 1], ref.counts[..., 1] + ref.counts[..., 3] + ref.counts[..., 4])
    for i, (n, name) in enumerate(zip(R.SUMS, ("pair_iou", "centre_err", "brier"))):
        assert got[n].dtype == torch.float64 and (np.abs(got[n].numpy() - ref.sums[..., i]) <= bar[name] * terms[i]).all(), n
    want = R.pooled(ref.counts, np.stack([got[n].numpy() for n in R.SUMS], -1), ref.lane_counts)
    for n, v in want.items():
        a = np.asarray(got[n], np.float64)
        assert a.shape == np.shape(v) and np.allclose(a, v, rtol=1e-12, atol=0.0, equal_nan=True), (n, a, v)
    assert got["fde"] == got["ade"][-1] or (np.isnan(got["fde"]) and np.isnan(float(got["ade"][-1])))
    assert int(got["calls"].sum()) == calls * B


CALLS = dict(forecast=lambda st, **kw: st.forecast(FH, samples=S, lane=True, seed=3, **kw),
             tracks=lambda st, **kw: st.tracks(LAG, lane=True, **kw))
FRAMES = dict(forecast=FH, tracks=LAG)


@pytest.mark.parametrize("kind", ["forecast", "tracks"])
def test_the_score_equals_the_reference_and_changes_nothing_else(stepped, kind):
    st, _ = stepped
    st._traj.clear()
    F = FRAMES[kind]
    plain = host(CALLS[kind](st))
    assert "score" not in plain["lane"] and not st._traj                # without truth nothing is launched, nothing is kept
    truth = _make_truth(plain["lane"], F, 21, kind == "tracks")
    if kind == "tracks":                                                # the anchor defaults to the newest frame
        truth = {n: v for n, v in truth.items() if not n.startswith("anchor")}
    got = host(CALLS[kind](st, truth=truth))
    score = got["lane"].pop("score")
    same_bits(plain, got)                                              # every other output: the same bits
    if kind == "tracks":
        truth = dict(truth, anchor_box=truth["box"][-1], anchor_present=truth["present"][-1], anchor_valid=truth["valid"][-1])
    ref, bar = _reference(got["lane"], truth)
    _check(score, ref, bar)
    assert score["state"].shape == (F, B, G) and score["link"].shape == (B, G) and score["count_map"].shape == (F, B)
    tot = dict(zip(R.COUNTS, ref.counts.sum((0, 1)).tolist()))
    lanes = dict(zip(R.LANE_COUNTS, ref.lane_counts.sum(0).tolist()))
    print(kind, tot, lanes, {n: "{:.3g}".format(v) for n, v in bar.items()})
    assert tot["pairs"] > 0 and tot["gone"] > 0 and tot["frames"] < F * B and lanes["anchor_truth"] > lanes["linked"] > 0
    holes = (got["lane"]["alive"] == 0) & (got["lane"]["presence"] != 0)[None]      # an object of the lane that no path holds at a frame
    print(kind, "frames of lane objects without a living path:", int(holes.sum()))
    assert tot["lost"] > 0 or not holes.any()
    if kind == "tracks":                                                # objects born inside the window: no path holds them before
        assert holes.any() and tot["lost"] > 0
    # the accumulators after one call, after a second one, and after reset=True
    one = st.trajectory_score(kind)
    _check_accumulated(one, ref, bar, 1)
    again = host(CALLS[kind](st, truth=truth))
    same_bits(dict(got, lane=dict(got["lane"], score=score)), again)
    ref2, _ = _reference(got["lane"], truth, acc=dict(counts=ref.counts, sums=ref.sums, lane_counts=ref.lane_counts))
    assert np.array_equal(ref2.counts, 2 * ref.counts)
    two = st.trajectory_score(kind, reset=True)
    _check_accumulated(two, ref2, bar, 2)
    zero = st.trajectory_score(kind)
    assert all(not zero[n].any() for n in R.COUNTS + R.SUMS + R.LANE_COUNTS)
    assert all(np.isnan(np.asarray(zero[n], np.float64)).all() for n in ("ade", "fde", "mean_iou", "hit_rate", "brier", "count_accuracy", "link_rate"))
    # another F starts fresh accumulators and drops the old
    if kind == "forecast":
        st.forecast(FH, samples=S, lane=True, seed=3, truth=truth)
        short = {n: (v[:2] if n in ("box", "present", "valid") else v) for n, v in truth.items()}
        st.forecast(2, samples=S, lane=True, seed=3, truth=short)
        fresh = st.trajectory_score("forecast")
        assert fresh["frames"].shape == (2, B) and int(fresh["calls"].sum()) == B


@pytest.mark.parametrize("kind", ["forecast", "tracks"])
def test_truth_equal_to_the_table_gives_iou_one_and_error_zero(stepped, kind):
    st, _ = stepped
    st._traj.clear()
    F = FRAMES[kind]
    lane = host(CALLS[kind](st))["lane"]
    living = (lane["alive"] > 0) & (lane["presence"] != 0)[None]
    truth = dict(box=np.where(living[..., None], lane["box_mean"], 0.0).astype(np.float32), present=living.astype(np.int32),
                 anchor_box=lane["box0"], anchor_present=(lane["presence"] != 0).astype(np.int32))
    score = host(CALLS[kind](st, truth=truth))["lane"]["score"]
    want = np.where(lane["presence"] != 0, np.arange(N)[None], -1)
    assert np.array_equal(score["link"], want) and (score["link_iou"][want >= 0] == 1.0).all()
    pairs = score["state"] == 1
    assert pairs.any() and np.array_equal(pairs, living) and (score["pair_iou"][pairs] == 1.0).all() and not score["centre_err"].any()
    assert (score["state"][~living & (want >= 0)[None]] == 0).all()     # where nothing lives the truth is absent: gone, never lost
    got = st.trajectory_score(kind)
    assert np.array_equal(got["hits"].numpy(), got["pairs"].numpy()) and int(got["pairs"].sum()) == int(pairs.sum()) and not got["lost"].any()
    assert not got["centre_err_sum"].any() and np.array_equal(got["iou_sum"].numpy(), got["pairs"].numpy().astype(np.float64))
    assert got["link_rate"] == 1.0 and (got["mean_iou"][got["pairs"].sum(1) > 0] == 1.0).all()
    if kind == "tracks":                                                # the newest frame is the anchor's: alive there is support
        assert (score["p_alive"][F - 1][want >= 0] == 1.0).all()


def test_tracks_and_forecast_between_the_same_two_steps_give_the_same_link(stepped):
    st, _ = stepped
    st._traj.clear()
    tk = host(CALLS["tracks"](st))["lane"]
    fc = host(CALLS["forecast"](st))["lane"]
    same_bits({n: tk[n] for n in ("obj_id", "presence", "box0")}, {n: fc[n] for n in ("obj_id", "presence", "box0")})
    t_tk, t_fc = _make_truth(tk, LAG, 33, True), _make_truth(fc, FH, 34, False)
    for n in ("anchor_box", "anchor_present"):                          # one anchor for both
        t_fc[n] = t_tk[n]
    a = host(CALLS["tracks"](st, truth=t_tk))["lane"]["score"]
    b = host(CALLS["forecast"](st, truth=t_fc))["lane"]["score"]
    same_bits({n: a[n] for n in ("link", "link_iou")}, {n: b[n] for n in ("link", "link_iou")})
    assert (a["link"] >= 0).any() and (a["link"] == -1).any()
    both = (st.trajectory_score("tracks"), st.trajectory_score("forecast"))      # each kind keeps accumulators of its own
    assert both[0]["frames"].shape == (LAG, B) and both[1]["frames"].shape == (FH, B)
    assert np.array_equal(both[0]["linked"].numpy(), both[1]["linked"].numpy())


def test_link_ids_keeps_a_truth_with_the_identity_the_score_last_matched(stepped):
    st, last = stepped
    st._traj.clear()
    memory = st._score["last_id"].cpu().numpy()
    assert (memory >= 0).any()
    lane = host(CALLS["forecast"](st))["lane"]
    truth = _make_truth(lane, FH, 41, False)
    truth["anchor_box"], truth["anchor_present"] = last["box"][0], last["present"][0]      # the truth of the last stepped frame
    for keep, kw in ((None, {}), (memory, dict(link_ids=True))):
        st._traj.clear()
        score = host(CALLS["forecast"](st, truth=truth, **kw))["lane"]["score"]
        ref, bar = _reference(lane, truth, keep)
        _check(score, ref, bar)
        assert (ref.link >= 0).any()
    assert np.array_equal(st._score["last_id"].cpu().numpy(), memory)   # read, never written
    three = dict(box=truth["box"][:, :, :3], present=truth["present"][:, :, :3], anchor_box=truth["anchor_box"][:, :3],
                 anchor_present=truth["anchor_present"][:, :3])
    with pytest.raises(ValueError, match="link_ids is for a stream with score=True and the same G"):
        st.forecast(FH, samples=S, lane=True, truth=three, link_ids=True)
