"""-m gpu: stream scoring inside the streaming pass (include/sqair_hip.h: sqair_set_score; SqairStream(estimate=True, score=True)), on
the configuration and batch of tests/test_estimate_stream.py (B = 4, K = 3, N = 3, 50 x 50), a dozen frames each.

A tracker with random parameters does not follow the generator's truth, so the truth is made from a first, unscored run with the same
seed: its lane boxes, jittered by 1.5 px, put into G = 4 truth slots by a rotation that changes every four frames (so a truth slot
meets another identity), a fifth of them dropped (false positives) and a truth added in the spare slot in a third of the frames
(misses).  Checked here: the score fields of ``out["lane"]`` and ``score()`` equal the float64 reference (tests/score_ref.py) applied
to the step's own lane outputs -- integers exactly, ``match_iou`` within four times the measured error of the fp32 restatement of
sq_box_iou on those boxes; no frame of these runs is fragile (asserted), so nothing is left out --; switching the score on changes
nothing else, bit for bit, and adds exactly one graph node; graph replay and eager steps give the same bits; three frames per step;
with SMC; with a coasted lane; ``reset()`` clears the identity memory and keeps the counters; a step without ``truth`` changes no
accumulator; ``score(reset=True)`` starts the counters again."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import score_ref as R
from tests.stream_harness import EST_KEYS, OUTS, SCORE, SMC_OUTS, host, run, same_bits, setup, stream, unscored_truth

pytestmark = pytest.mark.gpu

SCORE_KEYS = set(_capi.SCORE_FIELDS)
HW, FLAGS, B, G, N, IOU = SCORE.HW, SCORE.FLAGS, SCORE.B, SCORE.G, SCORE.N, SCORE.IOU
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)


def _setup(T, seed=11):
    return setup(FLAGS, B, T, HW, seed)


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=IOU, **kw)


def _scored(F, P, **kw):
    return _stream(F, P, score=True, score_iou=IOU, score_truth=G, **kw)


class _Ref(object):
    """The reference carried along a scored stream: its accumulators and memory, the figures seen."""

    def __init__(self):
        self.counts = self.iou_sum = self.last_id = None
        self.worst = self.tol = 0.0

    def step(self, o, truth):
        lane = o["lane"]
        T = lane["map_count"].shape[0]
        if truth is None:
            truth = dict(box=np.zeros((T, B, G, 4), np.float32), present=np.zeros((T, B, G), np.int32), valid=np.zeros((T, B), np.int32))
        args = dict(box=lane["box"], presence=lane["presence"], obj_id=lane["obj_id"], map_count=lane["map_count"],
                    truth_box=truth["box"], truth_present=truth["present"], truth_valid=truth["valid"], iou_min=IOU)
        ref = R.score(counts=self.counts, iou_sum=self.iou_sum, last_id=self.last_id, **args)
        first = R.fragile_from(ref.iou, lane["presence"], lane["map_count"], truth["present"], truth["valid"], IOU)
        assert (first == T).all(), "a fragile frame: a decision within 1e-5 of a threshold"
        self.counts, self.iou_sum, self.last_id = ref.counts, ref.iou_sum, ref.last_id
        for n in _capi.SCORE_INT_FIELDS:
            assert lane[n].dtype == np.int32 and np.array_equal(lane[n], getattr(ref, n)), (n, lane[n], getattr(ref, n))
        tol = 4.0 * R.iou32_error(truth["box"] * (truth["present"] != 0)[..., None], lane["box"])      # (over boxes that are boxes)
        err = float(np.abs(lane["match_iou"].astype(np.float64) - ref.match_iou).max())
        self.worst, self.tol = max(self.worst, err), max(self.tol, tol)
        assert tol < 1e-5 and err <= tol, (err, tol)
        return ref

    def check_score(self, got):
        for i, n in enumerate(R.COUNTS):
            assert got[n].dtype == torch.int64 and np.array_equal(got[n].numpy(), self.counts[:, i]), (n, got[n], self.counts[:, i])
        tp = self.counts[:, 3]
        assert got["iou_sum"].dtype == torch.float64 and (np.abs(got["iou_sum"].numpy() - self.iou_sum) <= self.tol * tp).all()
        want = R.pooled(self.counts, got["iou_sum"].numpy())
        for n, v in want.items():
            assert abs(got[n] - v) <= 1e-12 or (np.isnan(got[n]) and np.isnan(v)), (n, got[n], v)

    def totals(self):
        return dict(zip(R.COUNTS, self.counts.sum(0).tolist()))


def _truth_for(F, P, obs, noise, observed=None, **kw):
    return unscored_truth(_stream(F, P, **kw), obs, noise, kw.get("frames_per_step", 1), observed)


# ---- 1. nothing else changes; one node more; graph == eager; against the reference, with SMC -------------------------------------------
def test_the_score_changes_nothing_else_and_equals_the_reference():
    T = 12
    F, P, obs, noise = _setup(T)
    truth, a = _truth_for(F, P, obs, noise, **SMC)
    off, on, eager = _stream(F, P, **SMC), _scored(F, P, **SMC), _scored(F, P, use_graph=False, **SMC)
    ref = _Ref()
    went = 0
    for t in range(T):
        f = slice(t, t + 1)
        o, b, c = (host(s.step(obs[f], noise=noise[f], **kw)) for s, kw in ((off, {}), (on, dict(truth=truth[t])), (eager, dict(truth=truth[t]))))
        assert set(o["lane"]) == EST_KEYS and set(b["lane"]) == EST_KEYS | SCORE_KEYS
        same_bits(o, b, OUTS + SMC_OUTS, t)
        same_bits(o["lane"], b["lane"], EST_KEYS, t)
        same_bits(a[t]["lane"], b["lane"], EST_KEYS, (t, "the run the truth was made from"))
        for k in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src"):
            assert torch.equal(getattr(off, k), getattr(on, k)), (t, k)
        same_bits(b["lane"], c["lane"], b["lane"].keys(), (t, "eager"))      # eager and graph: the same bits
        assert b["lane"]["truth_match"].shape == (1, B, G) and b["lane"]["tp"].shape == (1, B)
        ref.step(b, truth[t])
        went += int(b["resampled"].sum())
    assert went > 0
    assert on.core.graph_nodes() == off.core.graph_nodes() + 1
    got, got_eager = on.score(), eager.score()
    ref.check_score(got)
    assert all(torch.equal(got[n], got_eager[n]) for n in R.COUNTS + ("iou_sum",))      # the fp64 sum too: the same bits
    for k in ("counts", "iou_sum", "last_id"):
        assert torch.equal(on._score[k], eager._score[k]), k
    assert np.array_equal(on._score["last_id"].cpu().numpy(), ref.last_id)
    tot = ref.totals()
    print("smc", tot, "match_iou worst error {:.3g}, allowed {:.3g}".format(ref.worst, ref.tol), {n: got[n] for n in ("mota", "motp", "count_accuracy")})
    assert min(tot["tp"], tot["fn"], tot["fp"], tot["idsw"]) > 0, tot      # all four events occur
    assert tot["frames"] < T * B                                          # and some frames had no truth
    for s in (off, on, eager):
        s.close()


# ---- 2. without SMC; three frames per step --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resample,Ts", [(None, 1), (None, 3), ("systematic", 3)], ids=["plain", "plain_T3", "smc_T3"])
def test_score_against_reference(resample, Ts):
    T = 12
    F, P, obs, noise = _setup(T, seed=3)
    kw = dict(frames_per_step=Ts, resample=resample, ess_frac=0.5, seed=17)
    truth, _ = _truth_for(F, P, obs, noise, **kw)
    st = _scored(F, P, **kw)
    ref = _Ref()
    for s, o in enumerate(run(st, obs, noise, Ts, truth=truth)):
        ref.step(o, truth[s])
    ref.check_score(st.score())
    tot = ref.totals()
    print(resample, Ts, tot, "match_iou worst error {:.3g}, allowed {:.3g}".format(ref.worst, ref.tol))
    assert min(tot["tp"], tot["fn"], tot["fp"]) > 0, tot
    st.close()


# ---- 3. a coasted lane is scored when its truth is valid -------------------------------------------------------------------------------
def test_a_coasted_lane_needs_no_case_of_its_own():
    T = 12
    F, P, obs, noise = _setup(T, seed=13)
    rng = np.random.default_rng(2)
    observed = np.stack([np.ones(B, bool) if t < 2 else rng.uniform(size=B) < 0.6 for t in range(T)])
    truth, _ = _truth_for(F, P, obs, noise, observed=observed, missing=True)
    st = _scored(F, P, missing=True)
    ref = _Ref()
    scored_coasted = 0
    for t, o in enumerate(run(st, obs, noise, truth=truth, observed=observed)):
        ref.step(o, truth[t])
        scored_coasted += int((~observed[t] & (truth[t]["valid"][0] != 0) & (o["lane"]["tp"][0] >= 0)).sum())
    ref.check_score(st.score())
    assert scored_coasted > 4 and ref.totals()["tp"] > 0
    st.close()


# ---- 4. reset, steps without truth, score(reset=True) ----------------------------------------------------------------------------------
def test_reset_clears_the_memory_and_a_step_without_truth_changes_no_accumulator():
    T = 12
    F, P, obs, noise = _setup(T, seed=19)
    truth, _ = _truth_for(F, P, obs, noise)
    truth[5] = truth[6] = None                # two steps without truth
    st = _scored(F, P)
    ref = _Ref()
    state = lambda: {k: st._score[k].clone() for k in ("counts", "iou_sum", "last_id")}
    for t in range(T):
        f = slice(t, t + 1)
        if t in (4, 9):                       # (the unscored run was not reset: from here on the truth is simply another scene)
            lanes = [1] if t == 4 else [0, 3]
            before = state()
            st.reset(lanes)
            after = state()
            assert torch.equal(before["counts"], after["counts"]) and torch.equal(before["iou_sum"], after["iou_sum"])
            assert (after["last_id"][lanes] == -1).all()
            keep = [b for b in range(B) if b not in lanes]
            assert torch.equal(before["last_id"][keep], after["last_id"][keep]) and (before["last_id"][keep] >= 0).any()
            ref.last_id[lanes] = -1
        before = state()
        o = host(st.step(obs[f], noise=noise[f], **({} if truth[t] is None else dict(truth=truth[t]))))
        if truth[t] is None:
            after = state()
            assert all(torch.equal(before[k], after[k]) for k in before), t
            assert all((o["lane"][n] == -1).all() for n in _capi.SCORE_INT_FIELDS) and not o["lane"]["match_iou"].any()
        ref.step(o, truth[t])
    got = st.score(reset=True)
    ref.check_score(got)
    assert ref.totals()["tp"] > 0 and ref.totals()["frames"] > 0
    again = st.score()
    assert all(not again[n].any() for n in R.COUNTS + ("iou_sum",)) and all(np.isnan(again[n]) for n in ("mota", "motp", "count_accuracy"))
    assert np.array_equal(st._score["last_id"].cpu().numpy(), ref.last_id)      # the memory stays
    st.close()


def test_step_argument_errors():
    F, P, obs, noise = _setup(1)
    st = _stream(F, P)
    with pytest.raises(ValueError, match="truth is for a stream with score=True"):
        st.step(obs[:1], truth=dict(box=np.zeros((1, B, G, 4)), present=np.zeros((1, B, G))))
    with pytest.raises(ValueError, match="keeps no score"):
        st.score()
    st.close()
    st = _scored(F, P)
    with pytest.raises(ValueError, match=r"truth\['box'\] of shape"):
        st.step(obs[:1], truth=dict(box=np.zeros((1, B, G + 1, 4)), present=np.zeros((1, B, G))))
    with pytest.raises(ValueError, match="must be a dict with box, present"):
        st.step(obs[:1], truth=dict(box=np.zeros((1, B, G, 4))))
    st.step(obs[:1], noise=noise[:1], truth=dict(box=np.zeros((B, G, 4)), present=np.zeros((B, G))))      # [B, ...] at T' = 1
    assert int(st.score()["frames"].sum()) == B
    st.close()
