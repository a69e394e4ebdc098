"""-m gpu: track log scoring on a stream (SqairStream(estimate=True, identity=True, tracklog=L, tracklog_truth=G);
``track_log(lag, score=True)``; include/sqair_hip.h: sqair_lane_tracklog_score), B = 4, K = 3 or 5, N = 3, 50 x 50, a dozen frames of
make_sequences, the truth cut from an unscored run (tests/stream_harness.py: make_truth, G = 4).

Checked here: ``tracklog_truth=G`` leaves every output bit, the log's bytes and ``sqair_graph_nodes`` of the ``tracklog`` stream
unchanged, and ``track_log(lag)`` without ``score`` returns that stream's bits; the truth ring gathered into window order gives the
reference's score (tests/tracklog_score_ref.py) of the truth the steps were given, on the solve's own outputs read back -- counters,
``match`` exactly, ``assign`` as the IDF's is judged, ``sums`` within the bars measured on that run --, with the ring wrapped
(L = 8 < 12 frames), for both matchings, over windows shorter than the ring, before the first step and over steps without truth;
single steps equal chunks of three bit for bit; ``reset([1])`` mid-stream leaves the ring alone and takes lane 1's earlier frames out
of the score; composed with ``score=True`` (the same G), ``missing=True``, SMC and ``identity_match="optimal"`` the step's outputs
and the score's accumulators keep their bits."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import tracklog_score_cases as SC
from tests import tracklog_score_ref as SR
from tests.stream_harness import OUTS, SCORE, host, make_truth, run, same_bits, same_bytes, setup, stream

pytestmark = pytest.mark.gpu

HW = SCORE.HW
FLAGS = dict(k_particles=5, n_steps_per_image=3)
B, N, G, L, TRACKS = SCORE.B, SCORE.N, SCORE.G, 8, 6
IDENT = dict(identity=True, identity_iou=0.3, identity_reid_dist=4.0, identity_max_age=3)
LOG = dict(tracklog=L, tracklog_tracks=TRACKS)
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)
T = 12
IOU = 0.5
K = {n: i for i, n in enumerate(SR.COUNTS)}
S = {n: i for i, n in enumerate(SR.SUMS)}
MODES = ("greedy", "optimal")


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=0.5, **kw)


def _flat(log):
    out = {}
    for k, v in log.items():
        if isinstance(v, dict):
            out.update({k + "." + kk: vv for kk, vv in _flat(v).items()})
        else:
            out[k] = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return out


def _frames(truth, Ts=1):
    """Per-step truth dicts (None: a step without truth) as one entry per frame."""
    out = []
    for t in truth:
        out += [None] * Ts if t is None else [{k: v[f] for k, v in t.items()} for f in range(Ts)]
    return out


def _window(frames, lag):
    """The truth the steps were given, in window order: frame n - lag + f; invalid before the first frame and where no truth was given."""
    n = len(frames)
    w = dict(truth_box=np.zeros((lag, B, G, 4), np.float32), truth_present=np.zeros((lag, B, G), np.int32), truth_valid=np.zeros((lag, B), np.int32))
    for f in range(lag):
        t = n - lag + f
        if t >= 0 and frames[t] is not None:
            w["truth_box"][f], w["truth_present"][f], w["truth_valid"][f] = frames[t]["box"], frames[t]["present"], frames[t]["valid"]
    return w


def _check(st, frames, case, lag=None, mode="greedy", tracks=TRACKS):
    """track_log(lag, score=True) against the reference's score of the given truth on the solve's own outputs."""
    lag = st.lane.log_L if lag is None else lag
    log = st.track_log(lag=lag, score=True, score_iou=IOU, score_match=mode)
    torch.cuda.synchronize()
    table = {k: st.lane._log_out["out"][k].cpu().numpy() for k in SR.TABLE}
    truth = _window(frames, lag)
    ref = SR.score(table, st._tracklog["log_valid"].cpu().numpy(), truth, IOU, mode)
    assert SR.fragile(ref, truth, IOU) == [], "a candidate within 1e-5 of a decision: move the truth's seed"
    sc = log["score"]
    assert tuple(sc) == SR.VIEWS
    bars = SR.bars(ref)
    worst = {n: 0.0 for n in SR.SUMS}
    for v, name in enumerate(SR.VIEWS):
        r = sc[name]
        for n in SR.COUNTS:
            assert r[n].dtype == torch.int64 and r[n].tolist() == ref.counts[:, v, K[n]].tolist(), (case, name, n, r[n], ref.counts[:, v, K[n]])
        assert r["match"].shape == (lag, B, G) and np.array_equal(r["match"].numpy(), ref.match[v]), (case, name)
        assert r["assign"].shape == (B, G) and r["match_iou"].dtype == torch.float32
        for b in range(B):
            SR.check_assign(ref.ov[b, v], r["assign"][b].numpy(), int(ref.counts[b, v, K["idtp"]]))
        for n in SR.SUMS:
            err = np.abs(r[n].numpy() - ref.sums[:, v, S[n]])
            worst[n] = max(worst[n], float(err.max()))
            assert r[n].dtype == torch.float64 and (err <= bars[:, v, S[n]]).all(), (case, name, n, err, bars[:, v, S[n]])
        for n, want in SR.pooled(ref.counts, r_sums(sc), v).items():
            assert (np.isnan(r[n]) and np.isnan(want)) or abs(r[n] - want) <= 1e-14 * max(1.0, abs(want)), (case, name, n, r[n], want)
    tot = dict(zip(SR.COUNTS, ref.counts.sum(0)[3].tolist()))
    print(case, mode, "lag", lag, "smooth_filled", tot, "term errors", ref.term_err, "the stream's worst error per sum", worst)
    SC.record("stream", case + "_" + mode, lag=lag, term_error=ref.term_err, kernel_error=worst,
              bars={n: float(bars[..., i].max()) for n, i in S.items()}, counts=tot)
    return log, ref


def r_sums(sc):
    """The stream's own sums [B, 4, 5] (the pooled figures are formed from what the stream read back)."""
    return np.stack([np.stack([sc[name][n].numpy() for n in SR.SUMS], -1) for name in SR.VIEWS], 1)


def _truth_of(F, P, obs, noise, Ts=1, **kw):
    """make_truth of an unscored run of the same stream."""
    st = _stream(F, P, frames_per_step=Ts, **IDENT, **kw)
    truth = make_truth(run(st, obs, noise, Ts), Ts)
    st.close()
    return truth


# ---- 1. the truth ring moves no bit; ring plus gather equal the reference ------------------------------------------------------------
def test_the_ring_moves_no_bit_and_the_score_is_the_references():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 11)
    truth = _truth_of(F, P, obs, noise)
    plain, on = _stream(F, P, **IDENT, **LOG), _stream(F, P, tracklog_truth=G, **IDENT, **LOG)
    with pytest.raises(ValueError, match=r"^SqairStream.step: truth is for a stream with score=True"):
        plain.step(obs[:1], noise=noise[:1], truth=truth[0])
    empty = on.track_log(score=True)["score"]                                 # before the first step: nothing is scored
    assert all(not empty[v][n].any() for v in SR.VIEWS for n in SR.COUNTS) and (empty["smooth"]["match"] == -1).all()
    a, b = run(plain, obs, noise), run(on, obs, noise, truth=truth)
    for t, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, None, (t, "tracklog_truth"))
    assert on.core.graph_nodes() == plain.core.graph_nodes()                  # no node is added
    for n in _capi.TRACKLOG_FIELDS:
        assert torch.equal(plain._tracklog[n].view(torch.uint8), on._tracklog[n].view(torch.uint8)), n
    for k in plain._ident:
        assert torch.equal(plain._ident[k].view(torch.uint8), on._ident[k].view(torch.uint8)), k
    want = _flat(plain.track_log())
    same_bytes(_flat(on.track_log()), want, None, "track_log() without score")
    assert on._truth_ring["truth_box"].shape == (L, B, G, 4) and on.lane.ring_frames == T and T > L      # the ring wrapped
    frames = _frames(truth)
    for mode in MODES:
        log, ref = _check(on, frames, "single_steps", mode=mode)
        scored = {k: v for k, v in _flat(log).items() if not k.startswith("score.")}
        same_bytes(scored, want, None, "track_log(score=True) but for its score")
        assert ref.counts[:, 3, K["tp"]].sum() > 0 and ref.counts[:, 0, K["frames"]].sum() > 0
    _check(on, frames, "lag_5", lag=5)
    for s in (plain, on):
        s.close()


# ---- 2. single steps equal chunks of three; steps without truth ------------------------------------------------------------------------
def test_single_steps_equal_chunks_of_three_and_steps_without_truth():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 3)
    truth3 = _truth_of(F, P, obs, noise, 3)
    truth3[2] = None                                                          # frames 6-8: a step without truth
    frames = _frames(truth3, 3)
    truth1 = [None if f is None else {k: v[None] for k, v in f.items()} for f in frames]
    one = _stream(F, P, frames_per_step=1, tracklog_truth=G, **IDENT, **LOG)
    three = _stream(F, P, frames_per_step=3, tracklog_truth=G, **IDENT, **LOG)
    run(one, obs, noise, 1, truth=truth1)
    run(three, obs, noise, 3, truth=truth3)
    for n in _capi.TRACKLOG_TRUTH_FIELDS:
        assert torch.equal(one._truth_ring[n].view(torch.uint8), three._truth_ring[n].view(torch.uint8)), n
    assert not three._truth_ring["truth_valid"][[6, 7, 0]].any()              # frames 6, 7, 8 at positions 6, 7, 0
    log, ref = _check(three, frames, "chunks_of_three")
    assert (ref.counts[:, 0, K["frames"]] <= L - 3).all() and ref.counts[:, 0, K["frames"]].sum() > 0       # (frames 6, 7, 8 are in the window)
    same_bytes(_flat(one.track_log(score=True, score_iou=IOU)), _flat(log), None, "single steps against chunks")
    same_bytes(_flat(one.track_log(lag=5, score=True, score_match="optimal")), _flat(three.track_log(lag=5, score=True, score_match="optimal")),
               None, "lag 5, optimal")
    one.close()
    three.close()


# ---- 3. reset ---------------------------------------------------------------------------------------------------------------------------
def test_reset_leaves_the_ring_alone_and_takes_the_lanes_earlier_frames_out():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 19)
    truth = _truth_of(F, P, obs, noise)
    st = _stream(F, P, tracklog_truth=G, **IDENT, **LOG)

    def before(s):
        if s == 7:
            was = {n: t.clone() for n, t in st._truth_ring.items()}
            st.reset([1])
            torch.cuda.synchronize()
            assert all(torch.equal(was[n].view(torch.uint8), st._truth_ring[n].view(torch.uint8)) for n in was) and st.lane.ring_frames == 7
            sc = st.track_log(score=True)["score"]["smooth_filled"]
            assert sc["frames"][1] == 0 and sc["frames"][[0, 2, 3]].sum() > 0
    run(st, obs, noise, before=before, truth=truth)
    log, ref = _check(st, _frames(truth), "reset")
    assert log["frame_index"][:, 1].tolist() == [-1] * (L - (T - 7)) + list(range(T - 7))
    assert (ref.counts[1, :, K["frames"]] <= T - 7).all() and ref.counts[0, 0, K["frames"]] > T - 7
    st.close()


# ---- 4. composed ------------------------------------------------------------------------------------------------------------------------
def test_composed_with_the_score_missing_smc_and_the_optimal_link():
    F, P, obs, noise = setup(SCORE.FLAGS, B, T, HW, 11)
    rng = np.random.default_rng(2)
    observed = np.stack([np.ones(B, bool) if t < 2 else rng.uniform(size=B) < 0.7 for t in range(T)])
    mk = lambda **kw: stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=0.5, missing=True, **SMC, **kw)
    plain = mk()
    truth = make_truth(run(plain, obs, noise, observed=observed), 1)
    plain.close()
    sc = dict(score=True, score_iou=SCORE.IOU, score_truth=G, score_ids="lane", identity_match="optimal", **IDENT, **LOG)
    off, on = mk(**sc), mk(tracklog_truth=G, **sc)
    a, b = (run(s, obs, noise, observed=observed, truth=truth) for s in (off, on))
    assert on.core.graph_nodes() == off.core.graph_nodes()
    for t, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, None, (t, "composed"))
    got, want = on.score(), off.score()
    assert all(torch.equal(got[n], want[n]) for n in _capi.SCORE_COUNTS) and torch.equal(got["iou_sum"], want["iou_sum"]) and int(got["tp"].sum()) > 0
    for n in _capi.TRACKLOG_FIELDS:
        assert torch.equal(off._tracklog[n].view(torch.uint8), on._tracklog[n].view(torch.uint8)), n
    for mode in MODES:
        _check(on, _frames(truth), "composed", mode=mode)
    for s in (off, on):
        s.close()
