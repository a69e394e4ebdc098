"""-m gpu: the track log inside the streaming pass (include/sqair_hip.h: sqair_set_tracklog; SqairStream(estimate=True, identity=True,
tracklog=L)), B = 4, K = 5, N = 3, 50 x 50, a dozen frames of make_sequences.

Checked here: ``tracklog=None`` is the identity stream -- every output, the lane answer, the blob, the SMC accumulators, the track
table bit for bit, the same ``sqair_graph_nodes`` --; with the log on there is exactly one node more and still every one of those bits;
graph replay and eager steps leave the same log; the log's bytes equal the reference's append (tests/tracklog_ref.py) of the steps' own
``lane_id``, ``track_len``, ``box`` and ``best_row`` collected on the host, and ``track_log()`` equals the reference's solve of it --
the integer outputs and ``size`` exactly, the filtered and smoothed states within the bars measured on that run; stepping one frame at
a time equals chunks of three on the log's bytes and on ``track_log()``; with ``motion=True`` the log's filtered velocity has the bits
of the steps' ``velocity``; ``reset([1])`` empties lane 1's log and no other; it composes with ``missing=True``, SMC,
``identity_match="optimal"`` and ``score_ids="lane"``, leaving their outputs' bits alone."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.lane import mot_rows
from tests import tracklog_cases as TC
from tests import tracklog_ref as R
from tests.stream_harness import EST_KEYS, OUTS, SMC_OUTS, SCORE, host, make_truth, run, same_bits, same_bytes, setup, stream, words

pytestmark = pytest.mark.gpu

ID_KEYS = {"lane_id", "id_how", "track_len"}
HW = (50, 50)
FLAGS = dict(k_particles=5, n_steps_per_image=3)
B, N, L, TRACKS = 4, 3, 8, 6
IDENT = dict(identity=True, identity_iou=0.3, identity_reid_dist=4.0, identity_max_age=3)
SCALARS = (0.25, 1.0, 16.0)
MOTION = dict(motion=True, motion_q=SCALARS[0], motion_r=SCALARS[1], motion_v0=SCALARS[2], motion_gate=3.0)
LOG = dict(tracklog=L, tracklog_tracks=TRACKS)
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)
CARRIED = ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src")
T = 12
EXACT = ("track_id", "n_tracks", "len0", "frame_index", "state", "size")


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=0.5, **kw)


def _device_log(st):
    torch.cuda.synchronize()
    return {n: st._tracklog[n].cpu().numpy() for n in _capi.TRACKLOG_FIELDS}


def _reference_log(outs, records=L, resets=None):
    """The reference's append of the steps' own lane outputs; ``resets``: {step: lanes} whose count is zeroed ahead of that step."""
    log = R.new_log(B, records, N)
    for s, o in enumerate(outs):
        for b in (resets or {}).get(s, ()):
            log["count"][b] = 0
        lane = o["lane"]
        log = R.append(log, lane["lane_id"], lane["track_len"], lane["best_row"], lane["box"])
    return log


def _flat(log):
    """A track_log() result as one flat {name: array} (smooth.centre, ...)."""
    out = {}
    for k, v in log.items():
        if isinstance(v, dict):
            out.update({k + "." + kk: vv.numpy() for kk, vv in v.items()})
        else:
            out[k] = v.numpy()
    return out


def _check(st, outs, case, records=L, lag=None, tracks=TRACKS, resets=None):
    """The stream's log against the reference's append, its track_log() against the reference's solve of that log."""
    want = _reference_log(outs, records, resets)
    got = _device_log(st)
    for n in _capi.TRACKLOG_FIELDS:
        assert got[n].dtype == want[n].dtype and np.array_equal(words(got[n]), words(want[n])), n
    lag = records if lag is None else lag
    ref = R.smooth(want, lag, tracks, *SCALARS)
    log = st.track_log(lag=lag, q=SCALARS[0], r=SCALARS[1], v0=SCALARS[2])
    for k in EXACT:
        w = getattr(ref, k)
        assert log[k].numpy().dtype == w.dtype and np.array_equal(words(log[k].numpy()), words(w)), (k, log[k], w)
    bars = R.bars(ref.err)
    errs = {}
    for name, states in (("filtered", ref.filt), ("smooth", ref.smooth)):
        d = log[name]
        assert set(d) == {"centre", "velocity", "sigma", "box"} and d["box"].shape == (lag, B, tracks, 4)
        errs[name] = max(float(np.abs(d["centre"].numpy() - states[..., 0]).max()), float(np.abs(d["velocity"].numpy() - states[..., 1]).max()))
        assert torch.equal(d["box"], torch.cat([d["centre"] - 0.5 * log["size"], log["size"]], -1))
        assert np.allclose(d["sigma"].numpy(), np.sqrt(np.maximum(states[..., 2], 0.0)), rtol=0, atol=bars["smooth" if name == "smooth" else "filt"] + 1e-6)
    print(case, "bars", bars, "the stream's error against float64", errs, "tracks", ref.n_tracks.tolist())
    TC.record("stream", case, bars=bars, kernel_error=errs, tracks=int(ref.n_tracks.sum()), states=[int((ref.state == k).sum()) for k in range(4)])
    assert errs["filtered"] <= bars["filt"] and errs["smooth"] <= bars["smooth"], (errs, bars)
    assert ref.n_tracks.sum() > 0 and (ref.state == R.SEEN).any()
    return log, ref


# ---- 1. off is the identity stream; on adds one node and moves no bit; the log is the steps' outputs ----------------------------------
def test_off_changes_nothing_on_adds_one_node_and_the_log_is_the_steps_outputs():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 11)
    ident, off = _stream(F, P, **SMC, **IDENT), _stream(F, P, tracklog=None, **SMC, **IDENT)
    on, eager = _stream(F, P, **SMC, **IDENT, **LOG), _stream(F, P, use_graph=False, **SMC, **IDENT, **LOG)
    outs = []
    for t in range(T):
        f = slice(t, t + 1)
        a, o, b, c = (host(s.step(obs[f], noise=noise[f])) for s in (ident, off, on, eager))
        assert set(b["lane"]) == EST_KEYS | ID_KEYS                          # the log adds no step output
        same_bits(a, o, None, (t, "off"))
        same_bits(a, b, None, (t, "on"))                                     # on: every output, the lane answer included
        same_bits(b, c, None, (t, "eager"))
        for k in CARRIED:
            assert torch.equal(getattr(ident, k), getattr(off, k)) and torch.equal(getattr(ident, k), getattr(on, k)), (t, k)
        outs.append(b)
    for k in ident._ident:
        assert all(torch.equal(ident._ident[k].view(torch.uint8), s._ident[k].view(torch.uint8)) for s in (off, on, eager)), k
    nodes = ident.core.graph_nodes()
    assert off.core.graph_nodes() == nodes and on.core.graph_nodes() == nodes + 1      # nothing launched; one node more
    assert not hasattr(off.lane, "tracklog_buf") and off.lane.tracklog is False
    same_bytes(_device_log(on), _device_log(eager), None, "replay against eager")
    log, ref = _check(on, outs, "smc_single_steps")
    same_bytes(_flat(log), _flat(eager.track_log(q=SCALARS[0], r=SCALARS[1], v0=SCALARS[2])), None, "track_log: replay against eager")
    assert (_device_log(on)["count"] == T).all() and T > L                   # the ring wrapped
    # the defaults: lag = L, the stream's motion scalars (their defaults here); the MOT rows of the smoothed boxes
    same_bytes(_flat(on.track_log()), _flat(log), None, "defaults")
    rows = mot_rows(log, 0)
    stepped = (ref.state[:, 0] == R.SEEN) | (ref.state[:, 0] == R.GAP)
    assert rows.shape == (int(stepped.sum()), 6) and set(rows[:, 1].astype(int)) <= set(ref.track_id[0].tolist())
    assert (np.diff(rows[:, 0]) >= 0).all() and rows[:, 0].min() >= T - L
    print("nodes", nodes, "+ 1")
    for s in (ident, off, on, eager):
        s.close()


# ---- 2. one frame at a time equals chunks of three ------------------------------------------------------------------------------------
def test_single_steps_equal_chunks_of_three():
    """Without SMC the two runs see the same rows; what the log records is compared first (motion_stream's note: the estimate's
    weights may differ in the last bit between the two, its boxes and best rows must not)."""
    F, P, obs, noise = setup(FLAGS, B, T, HW, 3)
    one, three = _stream(F, P, frames_per_step=1, **IDENT, **LOG), _stream(F, P, frames_per_step=3, **IDENT, **LOG)
    singles, chunks = run(one, obs, noise, 1), run(three, obs, noise, 3)
    for n in ("box", "best_row", "lane_id", "track_len"):
        assert np.array_equal(words(np.concatenate([o["lane"][n] for o in chunks])), words(np.concatenate([o["lane"][n] for o in singles]))), n
    same_bytes(_device_log(one), _device_log(three), None, "the log")
    log, _ = _check(three, chunks, "chunks_of_three")
    same_bytes(_flat(one.track_log(lag=5)), _flat(three.track_log(lag=5)), None, "track_log(lag=5)")
    same_bytes(_flat(one.track_log()), _flat(log), None, "track_log()")
    one.close()
    three.close()


# ---- 3. with the motion on: the velocity's bits ----------------------------------------------------------------------------------------
def test_with_the_motion_on_the_filtered_velocity_has_the_steps_bits():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 19)
    st = _stream(F, P, **IDENT, **MOTION, tracklog=16, tracklog_tracks=12)
    outs = run(st, obs, noise)
    log, ref = _check(st, outs, "motion", records=16, lag=T, tracks=12)      # (the defaults are the stream's motion scalars)
    same_bytes(_flat(st.track_log(lag=T)), _flat(log), None, "the stream's scalars")
    ids = np.concatenate([o["lane"]["lane_id"] for o in outs])
    vel = np.concatenate([o["lane"]["velocity"] for o in outs])
    got = log["filtered"]["velocity"].numpy()
    n = 0
    for b in range(B):
        for col in np.flatnonzero(ref.len0[b] == 1):
            for f in np.flatnonzero(ref.state[:, b, col] == R.SEEN)[1:]:
                t = int(ref.frame_index[f, b])
                j = int(np.flatnonzero(ids[t, b] == ref.track_id[b, col])[0])
                assert np.array_equal(got[f, b, col].view(np.uint32), vel[t, b, j].view(np.uint32)), (b, col, f)
                n += 1
    print("velocities compared as bits", n)
    assert n > 0
    st.close()


# ---- 4. reset ---------------------------------------------------------------------------------------------------------------------------
def test_reset_empties_that_lanes_log_and_no_other():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 19)
    st = _stream(F, P, **IDENT, **LOG)
    resets = {7: [1]}

    def before(s):
        if s in resets:
            was = _device_log(st)
            st.reset(resets[s])
            now = _device_log(st)
            assert now["count"].tolist() == [s, 0, s, s]
            assert all(np.array_equal(words(now[n]), words(was[n])) for n in _capi.TRACKLOG_FIELDS if n != "count")
            empty = st.track_log()
            assert (empty["frame_index"][:, 1] == -1).all() and empty["n_tracks"].tolist()[1] == 0 and not empty["state"][:, 1].any()
            assert (empty["track_id"][1] == -1).all() and (empty["frame_index"][-1, [0, 2, 3]] == s - 1).all()
    outs = run(st, obs, noise, before=before)
    log, ref = _check(st, outs, "reset", resets=resets)
    assert log["frame_index"][:, 1].tolist() == [-1] * (L - (T - 7)) + list(range(T - 7)) and (log["frame_index"][-1, [0, 2, 3]] == T - 1).all()
    st.close()


# ---- 5. composed ------------------------------------------------------------------------------------------------------------------------
def test_composed_with_missing_smc_the_optimal_link_and_the_score_on_lane_ids():
    F, P, obs, noise = setup(SCORE.FLAGS, SCORE.B, T, SCORE.HW, 11)
    rng = np.random.default_rng(2)
    observed = np.stack([np.ones(SCORE.B, bool) if t < 2 else rng.uniform(size=SCORE.B) < 0.7 for t in range(T)])
    mk = lambda **kw: stream((F, SCORE.HW, P), SCORE.B, outputs=OUTS, estimate=True, estimate_iou=0.5, missing=True, **SMC, **kw)
    plain = mk()
    truth = make_truth(run(plain, obs, noise, observed=observed), 1)
    plain.close()
    sc = dict(score=True, score_iou=SCORE.IOU, score_truth=SCORE.G, score_ids="lane", score_idf=True, score_hota=True,
              identity_match="optimal", **IDENT, **MOTION)
    off, on = mk(**sc), mk(**sc, **LOG)
    a, b = (run(s, obs, noise, observed=observed, truth=truth) for s in (off, on))
    assert on.core.graph_nodes() == off.core.graph_nodes() + 1
    for t, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, None, (t, "composed"))                               # every output of the step, the score's included
    for k in CARRIED:
        assert torch.equal(getattr(off, k), getattr(on, k)), k
    for k in off._ident:
        assert torch.equal(off._ident[k].view(torch.uint8), on._ident[k].view(torch.uint8)), k
    got, want = on.score(), off.score()
    assert all(torch.equal(got[n], want[n]) for n in _capi.SCORE_COUNTS) and int(got["tp"].sum()) > 0
    gi, wi = on.idf_score(), off.idf_score()
    assert all(torch.equal(gi[n], wi[n]) for n in ("idtp", "idfn", "idfp", "frames"))
    gh, wh = on.hota_score(), off.hota_score()
    assert all(torch.equal(gh[n], wh[n]) for n in ("tp", "fn", "fp", "loc", "frames"))
    want_log = _reference_log(b)
    dev = _device_log(on)
    for n in _capi.TRACKLOG_FIELDS:
        assert np.array_equal(words(dev[n]), words(want_log[n])), n
    log = on.track_log()
    assert int(log["n_tracks"].sum()) > 0 and torch.isfinite(log["smooth"]["box"]).all()
    for s in (off, on):
        s.close()


def test_call_errors():
    F, P, obs, noise = setup(FLAGS, B, 1, HW, 11)
    with pytest.raises(ValueError, match=r"^SqairStream: tracklog is for a stream with identity=True"):
        _stream(F, P, tracklog=8)
    st = _stream(F, P, **IDENT)
    with pytest.raises(ValueError, match=r"^SqairStream.track_log: the stream keeps no track log"):
        st.track_log()
    st.close()
    st = _stream(F, P, **IDENT, **LOG)
    assert st._tracklog["log_box"].shape == (B, L, N, 4) and st._tracklog["count"].dtype == torch.int64
    with pytest.raises(ValueError, match=r"^SqairStream.track_log: lag must be an integer in \[1, tracklog = 8\]"):
        st.track_log(lag=9)
    empty = st.track_log()                                                   # before the first step: nothing logged
    assert (empty["frame_index"] == -1).all() and not empty["n_tracks"].any() and not empty["state"].any()
    st.close()
