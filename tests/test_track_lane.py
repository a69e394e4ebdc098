"""-m gpu: the lane tracks of a stream (include/sqair_hip.h: sqair_history_trace_lane; SqairStream.tracks(lane=True)), at the small
configuration of tests/test_history.py: SMC streams with K in {1, 5}, a reset lane, a ring that wraps, lag < L, 2-frame chunks and a
stream with missing frames.

* Against fp64: the step outputs and the source maps are recorded on the host, tests/history_ref.py traces them, and
  tests/track_lane_ref.py turns the traced rows into the lane answer; the comparison and its bars are tests/track_lane_check.py's.
  The per-row part of the same call equals the plain trace bit for bit.
* Graph replay of the stream equals the eager stream in every bit of the lane answer.
* Concatenation: between the same two steps tracks(lane=True) and forecast(3, samples=4, lane=True) list the same objects in the
  same order -- best_row, weights, presence, obj_id, box0 and support are the same bits (both read the same start rows through the
  same device functions).
* alive is non-decreasing in f on these real streams: an id's presence along a path is one interval ending at F - 1.
* A stream that calls tracks(lane=True) between steps equals one that does not, in every step output, blob byte and accumulator."""
import numpy as np
import pytest
import torch

from sqair_amd.stream import SqairStream
from tests import history_ref as H
from tests import track_lane_check as TC
from tests import track_lane_ref as TL
from tests.stream_harness import FIELD_OF, OUTS, core, host, setup

pytestmark = pytest.mark.gpu

HW = (50, 50)
N = 3
IOU = 0.5
SHARED = ("best_row", "weights", "presence", "obj_id", "box0", "support")     # what the lane tracks and the lane forecast both list
B, STEPS, L = 3, 6, 4                                                         # L < STEPS: the ring wraps


def _setup(K, T, seed=11):
    return setup(dict(k_particles=K, n_steps_per_image=N), B, T, HW, seed)


def _core(F, P):
    return core(F, HW, P)


def _next_rows(st):
    """The map the next step imports through and the fp32 log weights that follow it: what forecast() and tracks() start from."""
    torch.cuda.synchronize()
    lws = st.log_weight_sum.cpu().numpy()
    if st.smc:
        return st._src.cpu().numpy().astype(np.int64), lws
    m = np.asarray(st.carried.pending(), dtype=np.int64)
    return m, np.where(m >= 0, lws[np.maximum(m, 0)], np.float32(0.0)).astype(np.float32)


def _drive(K, Tp=1, missing=False, use_graph=True, ess_frac=0.5, check=True):
    """One stream of STEPS steps of Tp frames; lane 1 is reset before step 3.  After every step, and once more with the reset armed,
    tracks(lag, lane=True) for lag < L and lag = L, checked against the reference, and the forecast; returns what the device gave."""
    F, P, obs, noise = _setup(K, STEPS * Tp)
    kw = dict(resample="systematic", ess_frac=ess_frac, seed=5)
    st = SqairStream(_core(F, P), B, outputs=OUTS, history=L, frames_per_step=Tp, use_graph=use_graph, missing=missing, **kw)
    rec = H.Recorder(B * K)
    rng = np.random.default_rng(3)
    out, totals = [], dict(decisions=0, skipped=0, stats_checked=0, objects=0, born_inside=0)

    def look(s):
        """What tracks(lane=True) and forecast(lane=True) say between the same two steps."""
        nxt, lw = _next_rows(st)
        for lag in (2, L):
            got = host(st.tracks(lag=lag, lane=True, lane_iou=IOU, table=False))
            out.append(got)
            if not check:
                continue
            want = H.trace(rec.steps, L, lag, K, nxt, None)
            for k, v in want.items():          # the per-row part of the call is the plain trace
                assert got[k].dtype == v.dtype and H.same_bits(got[k], v), (k, s, lag)
            lane = got["lane"]
            ref = TL.lane_tracks(want["where"], want["presence"], want["obj_id"], want["valid"], lw, K, HW, IOU)
            margins, counts = TC.check(lane, ref, want["where"], want["presence"], want["valid"], K, HW, IOU)
            for k in ("decisions", "skipped", "stats_checked"):
                totals[k] += counts[k]
            Fr = lag * Tp
            assert np.array_equal(lane["alive"][Fr - 1].view(np.uint32), lane["support"].view(np.uint32))
            # monotone alive: non-decreasing in f (a particle that holds the id at f holds it at f + 1: the same terms and more, added
            # in the same order)
            assert (np.diff(lane["alive"], axis=0) >= 0).all(), (s, lag)
            totals["objects"] += int((lane["presence"] != 0).sum())
            totals["born_inside"] += int(((lane["first_frame"] > 0) & (lane["presence"] != 0)).sum())
        # ---- concatenation with the forecast taken between the same two steps
        fc = host(st.forecast(3, samples=4, lane=True, lane_iou=IOU, outputs=("presence",)))["lane"]
        for name in SHARED:
            assert H.same_bits(got["lane"][name], fc[name]), (name, s, got["lane"][name], fc[name])
        out.append({k: fc[k] for k in SHARED})

    for s in range(STEPS):
        parent, _ = _next_rows(st)
        step_kw = dict(noise=noise[s * Tp:(s + 1) * Tp], uniforms=rng.uniform(size=B).astype(np.float32))
        if missing:
            step_kw["observed"] = rng.uniform(size=(Tp, B)) < 0.6 if s not in (0, 3) else np.ones((Tp, B), bool)
        o = host(st.step(obs[s * Tp:(s + 1) * Tp], **step_kw))
        rec.push(parent, **{k: o[v] for k, v in FIELD_OF.items()})
        look(s)
        if s == 2:                             # lane 1 starts a new clip at step 3: its next rows are fresh, it has no past and no objects
            st.reset([1])
            look(s)
            assert not out[-1]["presence"][1].any() and out[-1]["presence"][[0, 2]].any()
    st.close()
    return out, totals


@pytest.mark.parametrize("K,Tp,missing", [(5, 1, False), (1, 1, False), (5, 2, False), (5, 1, True)],
                         ids=["K5", "K1", "K5_chunks_T2", "K5_missing"])
def test_stream_lane_tracks_against_fp64_and_the_forecast(K, Tp, missing):
    out, totals = _drive(K, Tp, missing)
    print(totals)
    assert totals["decisions"] > 1 and totals["skipped"] <= 0.01 * totals["decisions"], totals
    assert totals["stats_checked"] > 0 and totals["objects"] > 0, totals


def test_graph_replay_equals_eager():
    runs = [_drive(5, 1, False, use_graph=g, check=False)[0] for g in (False, True)]
    assert len(runs[0]) == len(runs[1]) > 0
    for e, g in zip(*runs):
        assert set(e) == set(g)
        for k in e:
            if isinstance(e[k], dict):
                assert set(e[k]) == set(g[k])
                for n in e[k]:
                    assert H.same_bits(e[k][n], g[k][n]), (k, n)
            else:
                assert H.same_bits(e[k], g[k]), k


def test_lane_tracks_between_steps_change_nothing():
    K, T = 4, 6
    F, P, obs, noise = _setup(K, T, seed=23)
    kw = dict(resample="systematic", ess_frac=0.5, seed=3)
    a = SqairStream(_core(F, P), B, outputs=OUTS, history=4, **kw)
    b = SqairStream(_core(F, P), B, outputs=OUTS, history=4, **kw)
    for t in range(T):
        b.tracks(lag=1 + t % 4, lane=True)
        oa, ob = host(a.step(obs[t:t + 1], noise=noise[t:t + 1])), host(b.step(obs[t:t + 1], noise=noise[t:t + 1]))
        assert set(oa) == set(ob)
        for k in oa:
            assert H.same_bits(oa[k], ob[k]), (k, t)
        for n in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src"):
            assert H.same_bits(getattr(a, n).cpu().numpy(), getattr(b, n).cpu().numpy()), (n, t)
    # the two calls share the ring's trace scratch and nothing else: a plain trace after a lane trace is still the plain trace
    lane, plain = host(b.tracks(lag=3, lane=True, table=False)), host(b.tracks(lag=3, table=False))
    for k in plain:
        assert H.same_bits(lane[k], plain[k]), k
    assert "lane" in lane and "lane" not in plain
    with pytest.raises(ValueError, match=r"^SqairStream\.tracks: lane=True requires start='next'"):
        b.tracks(lane=True, start="last")
