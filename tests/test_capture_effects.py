"""-m gpu: the eager pre-pass of a capture has no effect of its own.  With the in-launch slot chain on (sqair_set_option "slot_chain"),
sqair_graph_capture runs one eager pass before the capture to upload the chain's tables; that pass imports the carried state and
writes nothing but the workspace and the outputs (sqair_amd/csrc/sqair_internal.h: sq_without_effects).  Were one of the pass's
effects left on in it, the first step of a graph stream would resample, push, estimate, link identities or score twice.

One stream with EVERY per-pass effect on at once -- SMC, history, a mask with one coasted lane, the estimate, the layers, the
identities and the score (counting its switches on the identities' ``lane_id``) -- on a chained core, on the configuration of tests/test_score_stream.py (B = 4, K = 3, N = 3, 50 x 50), six one-frame steps
with explicit noise, uniforms and truth; the truth is made as that file makes it, from a first unscored run.  The stream is run once
through the captured graph and once eagerly (which has no pre-pass): every step's outputs (``lane`` included), the SMC outputs,
``score()``, ``identities()`` and the track table's device buffers, ``tracks()``, the state blob, ``log_weight_sum`` and
``log_evidence`` must agree bit for bit, every lane must have counted each scored step exactly once, and every lane's identity must
have seen each step exactly once.  A first step pushed twice is invisible to ``tracks()``: its rows start fresh, so every path ends
at the newer copy, and after six steps a ring of four slots holds the same four steps either way, rotated by one slot.  So the ring
itself -- its push counter and its slots -- is compared as well.  What the integers should be is pinned elsewhere (tests/score_ref.py through
tests/test_score_stream.py); here the reference for the counters is the number of scored steps."""
import numpy as np
import pytest
import torch

from sqair_amd.model import SqairCore
from tests.stream_harness import OUTS, SCORE, SMC_OUTS, core as make_core, host, make_truth, same_bytes, setup, stream

pytestmark = pytest.mark.gpu

HW, FLAGS, B, G, IOU = SCORE.HW, SCORE.FLAGS, SCORE.B, SCORE.G, SCORE.IOU
STEPS = 6


def _run(F, P, obs, noise, uniforms, observed, truth, use_graph):
    core = make_core(F, HW, P, options={"slot_chain": 1})
    st = stream(core, B, outputs=OUTS, use_graph=use_graph, resample="systematic", ess_frac=0.5, seed=5, history=4, missing=True,
                estimate=True, estimate_iou=IOU, estimate_layers=True, score=truth is not None, score_iou=IOU, score_truth=G,
                identity=True, score_ids="row" if truth is None else "lane")
    outs = []
    for t in range(STEPS):
        kw = {} if truth is None else dict(truth=truth[t])
        outs.append(host(st.step(obs[t:t + 1], noise=noise[t:t + 1], uniforms=uniforms[t], observed=observed[t:t + 1], **kw)))
        core.check_chain()      # every chain launch of the step completed
    # the chain really ran: the workspace was carved for it (slot buffers kept apart per frame and slot, control blocks) ...
    plain = SqairCore(F, HW)
    assert core.lib.sqair_workspace_bytes(core.handle, 1, B) > plain.lib.sqair_workspace_bytes(plain.handle, 1, B)
    res = dict(outs=outs, state=st.state.clone(), log_weight_sum=st.log_weight_sum.clone(), log_evidence=st.log_evidence.clone(),
               tracks=st.tracks(), ring=st.carried.ring.clone(), nodes=core.graph_nodes() if use_graph else None,
               identities=st.identities(), track_table={n: t.clone() for n, t in st._ident.items()})
    if truth is not None:
        res["score"] = st.score()
    torch.cuda.synchronize()
    st.close()
    return res


def test_graph_and_eager_streams_agree_with_every_effect_on():
    F, P, obs, noise = setup(FLAGS, B, STEPS, HW)
    rng = np.random.default_rng(23)
    uniforms = rng.uniform(size=(STEPS, B)).astype(np.float32)
    observed = np.ones((STEPS, B), bool)
    observed[3, 1] = False      # one lane coasts in one step
    first = _run(F, P, obs, noise, uniforms, observed, None, True)
    truth = make_truth(first["outs"], 1)
    truth[0]["valid"][:] = 1      # (the step a pre-pass would repeat is scored in every lane)
    graph = _run(F, P, obs, noise, uniforms, observed, truth, True)
    eager = _run(F, P, obs, noise, uniforms, observed, truth, False)
    assert graph["nodes"] == first["nodes"] + 1, (first["nodes"], graph["nodes"])      # (the score's one node)
    for t in range(STEPS):
        assert set(OUTS + SMC_OUTS + ("lane", "observed")) <= set(graph["outs"][t])
        same_bytes(graph["outs"][t], eager["outs"][t], where=("step", t))
    for k in ("score", "identities", "track_table", "tracks", "ring", "state", "log_weight_sum", "log_evidence"):
        g, e = graph[k], eager[k]
        same_bytes(g if isinstance(g, dict) else {k: g}, e if isinstance(e, dict) else {k: e}, where=(k,))
    assert sum(int(o["resampled"].sum()) for o in graph["outs"]) > 0      # the resampler went
    assert not graph["outs"][3]["observed"][0, 1] and graph["outs"][3]["observed"].sum() == B - 1
    # every scored step -- a step whose truth is valid for the lane -- counted once per lane: a pre-pass that scored would count the
    # first step twice
    scored_steps = sum((tr["valid"][0] != 0).astype(np.int64) for tr in truth)
    for name, res in (("graph", graph), ("eager", eager)):
        sc = res["score"]
        counted = (sc["frames"] + sc["frames_invalid"]).numpy()
        print(name, "frames", sc["frames"].tolist(), "frames_invalid", sc["frames_invalid"].tolist(), "scored steps", scored_steps.tolist())
        assert np.array_equal(counted, scored_steps), (name, counted, scored_steps)
    # the identity's version of the same: every step seen once per lane, with or without objects -- a pre-pass that linked would
    # see the first step twice
    for name, res in (("graph", graph), ("eager", eager), ("first", first)):
        idn = res["identities"]
        seen = (idn["frames"] + idn["frames_invalid"]).numpy()
        print(name, "identity frames", idn["frames"].tolist(), "frames_invalid", idn["frames_invalid"].tolist(), "steps", STEPS)
        assert np.array_equal(seen, np.full(B, STEPS)), (name, seen, STEPS)
