"""-m gpu: IDF1 scoring inside the streaming pass (include/sqair_hip.h: sqair_set_idf; SqairStream(estimate=True, score=True,
score_idf=True)): B = 4, K = 5, N = 3, 50 x 50, SMC, identity=True, 24 frames.

The truth is cut from an unscored run's lane boxes the way tests/test_score_stream.py makes its truth (tests/stream_harness.py: make_truth) (jittered, rotated between the
slots every four frames, a fifth dropped, some added).  Checked here: ``idf_score()`` equals the reference (tests/idf_ref.py) fed the
steps' own lane outputs -- boxes, presences, id words, map_count and the score's truth_match --, every integer exactly; no frame of
these runs has a pair within the fp32 error of the threshold (asserted), so nothing is left out; with ``score_idf`` on nothing else
changes bit for bit and the graph has exactly one node more; graph replay and eager steps leave the same table; ``reset([j])`` closes
lane j's clip (clips = 1, table free) and leaves the other lanes' tables alone; ``idf_score(reset=True)`` starts again; three frames
per step with a coasted lane; with ``score_ids="lane"`` the table is keyed by ``lane_id``.  The run's IDF1 on ``lane_id`` and on
``obj_id`` are printed side by side; nothing is asserted about which is larger."""
import numpy as np
import pytest
import torch

from tests import idf_ref as R
from tests.stream_harness import IDF_IDS as P_IDS, OUTS, SCORE, SMC_OUTS, IdfRef, host, same_bits, setup, stream, unscored_truth

pytestmark = pytest.mark.gpu

HW, B, G, N, IOU = SCORE.HW, SCORE.B, SCORE.G, SCORE.N, SCORE.IOU
FLAGS = dict(k_particles=5, n_steps_per_image=N)
T = 24
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)


def _setup(seed=11):
    return setup(FLAGS, B, T, HW, seed)


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=IOU, identity=True, **dict(SMC, **kw))


def _scored(F, P, idf=True, **kw):
    return _stream(F, P, score=True, score_iou=IOU, score_truth=G, score_idf=idf, score_idf_ids=P_IDS, **kw)


def _truth(F, P, obs, noise, Ts=1, observed=None, **kw):
    return unscored_truth(_stream(F, P, frames_per_step=Ts, **kw), obs, noise, Ts, observed)[0]


def test_idf_changes_nothing_else_and_equals_the_reference():
    F, P, obs, noise = _setup()
    truth = _truth(F, P, obs, noise)
    off, on, eager = _scored(F, P, idf=False), _scored(F, P), _scored(F, P, use_graph=False)
    ref = IdfRef()
    with pytest.raises(ValueError, match="keeps no IDF1 table"):
        off.idf_score()
    for t in range(T):
        f = slice(t, t + 1)
        if t == 13:      # lane 1 starts a new clip (the truth's run was not reset: from here on it is simply another scene)
            before = {n: v.clone() for n, v in on._idf.items()}
            for s in (off, on, eager):
                s.reset([1])
            ref.close([1])
            after = on._idf
            keep = [0, 2, 3]
            assert all(torch.equal(before[n][keep], after[n][keep]) for n in before)
            assert (after["col_id"][1] == -1).all() and int(after["frames"][1]) == 0 and not after["row_frames"][1].any()
            assert int(after["totals"][1, 0]) == 1 and int(after["totals"][1, 1]) == int(before["frames"][1]) > 0
            ref.check_table(on)
        o, b, c = (host(s.step(obs[f], noise=noise[f], truth=truth[t])) for s in (off, on, eager))
        assert set(o["lane"]) == set(b["lane"])      # nothing per frame: IDF1 is not a per-frame quantity
        same_bits(o, b, OUTS + SMC_OUTS, t)
        same_bits(o["lane"], b["lane"], o["lane"].keys(), t)
        same_bits(b["lane"], c["lane"], b["lane"].keys(), (t, "eager"))
        for k in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src"):
            assert torch.equal(getattr(off, k), getattr(on, k)), (t, k)
        ref.step(b, truth[t])
    for k in ("counts", "iou_sum", "last_id"):
        assert torch.equal(off._score[k], on._score[k]), k
    for k in off._ident:
        assert torch.equal(off._ident[k], on._ident[k]), k
    assert on.core.graph_nodes() == off.core.graph_nodes() + 1
    ref.check_table(on)
    for n in on._idf:
        assert torch.equal(on._idf[n], eager._idf[n]), n      # eager and graph: the same table
    got = on.idf_score()
    tot = ref.check_score(got)
    ref.check_table(on)                                       # reading the score closes nothing
    got_eager = eager.idf_score()
    assert all(torch.equal(got[n], got_eager[n]) for n in R.TOTALS if n != "frag") and got["idf1"] == got_eager["idf1"]
    print("obj_id", tot, {n: got[n] for n in ("idf1", "idp", "idr", "mt_rate", "ml_rate", "frag", "exact")}, "idsw", int(on.score()["idsw"].sum()))
    assert tot["clips"] == B + 1 and tot["frames"] > 0 and min(tot["idtp"], tot["idfn"], tot["idfp"]) > 0 and tot["trajectories"] > G
    # reset=True: the totals from zero, every table free
    on.idf_score(reset=True)
    again = on.idf_score()
    assert all(not again[n].any() for n in R.TOTALS if n != "frag") and np.isnan(again["idf1"]) and (on._idf["col_id"] == -1).all()
    for s in (off, on, eager):
        s.close()


@pytest.mark.parametrize("ids", ["lane", "row"])
def test_three_frames_per_step_a_coasted_lane_and_the_table_keyed_by_lane_id(ids):
    F, P, obs, noise = _setup(seed=13)
    rng = np.random.default_rng(2)
    observed = np.stack([np.ones(B, bool) if t < 3 else rng.uniform(size=B) < 0.7 for t in range(T)])
    truth = _truth(F, P, obs, noise, Ts=3, observed=observed, missing=True)
    st = _scored(F, P, frames_per_step=3, missing=True, score_ids=ids)
    ref = IdfRef("lane_id" if ids == "lane" else "obj_id")
    coasted = 0
    for s in range(T // 3):
        f = slice(3 * s, 3 * s + 3)
        o = host(st.step(obs[f], noise=noise[f], truth=truth[s], observed=observed[f]))
        ref.step(o, truth[s])
        coasted += int((~observed[f] & (truth[s]["valid"] != 0) & (o["lane"]["tp"] >= 0)).sum())
    ref.check_table(st)
    got = st.idf_score()
    tot = ref.check_score(got)
    print("ids =", ids, tot, {n: got[n] for n in ("idf1", "idp", "idr", "mt_rate", "ml_rate", "frag", "exact")}, "idsw", int(st.score()["idsw"].sum()))
    assert coasted > 4 and tot["idtp"] > 0 and tot["clips"] == B
    st.close()
