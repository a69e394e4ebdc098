"""-m gpu: keep + optimal per-frame matching from the stream (SqairStream(score_match=..., identity_match=...), forecast(link_match=...);
include/sqair_hip.h: sqair_set_lane_match): B = 4, K = 5, N = 3, 50 x 50, SMC, 30 frames.

The truth is cut from an unscored run's lane boxes the way tests/test_score_stream.py makes its truth (tests/stream_harness.py: make_truth), with coarser jitter and two
truths on the lane's first object, so that truths compete.  Isolation: with ``score_match="optimal"`` every output other than the
score's (and the IDF table, which reads truth_match) is bit-identical to the greedy stream's and the graph has the same number of
nodes; with ``identity_match="optimal"`` the same holds for everything but the identity's outputs and table (the score reads obj_id
here, ``score_ids="row"``).  Graph replay equals eager steps, with SMC, one and three frames per step.  Against the references:
``score()``, ``idf_score()``, ``identities()`` and the forecast's link equal the references run on the steps' own lane outputs with
the device's matching judged and imposed (tests/match_ref.py: Judge, IdentityFollower); no frame of these runs has a candidate within
1e-5 of a threshold for the score (asserted); tp of a frame in the optimal stream is never below the greedy stream's."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import identity_ref as I
from tests import match_ref as M
from tests import score_ref as R
from tests import traj_score_ref as TR
from tests.stream_harness import IDF_IDS as P_IDS, OUTS, SCORE, SMC_OUTS, IdfRef, host, same_bits, setup, stream, unscored_truth

pytestmark = pytest.mark.gpu

HW, B, G, N, IOU = SCORE.HW, SCORE.B, SCORE.G, SCORE.N, SCORE.IOU
FLAGS = dict(k_particles=5, n_steps_per_image=N)
T = 30
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)
SCORE_KEYS = set(_capi.SCORE_FIELDS)
IDENT_KEYS = {"lane_id", "id_how", "track_len"}
JITTER = np.array([3.0, 3.0, 1.5, 1.5])      # px, on (y, x, h, w)
STATE = ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src")


def _setup(seed=11):
    return setup(FLAGS, B, T, HW, seed)


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=IOU, identity=True, **dict(SMC, **kw))


def _scored(F, P, **kw):
    return _stream(F, P, score=True, score_iou=IOU, score_truth=G, score_idf=True, score_idf_ids=P_IDS, **kw)


def _cut(outs, Ts, seed=7):
    """One ``truth`` dict per step from an unscored run's lane boxes: truth g = (j + shift) % N is object j's box moved by 3 px and
    resized by 1.5 px of jitter, present four times in five; truth N is a second truth on object 0, present half of the time."""
    rng = np.random.default_rng(seed)
    truth = []
    for s, o in enumerate(outs):
        lane = o["lane"]
        box, present = np.zeros((Ts, B, G, 4), np.float32), np.zeros((Ts, B, G), np.int32)
        for k in range(Ts):
            shift = ((s * Ts + k) // 4) % 2
            for b in range(B):
                for j in range(N):
                    g = (j + shift) % N
                    box[k, b, g] = lane["box"][k, b, j] + JITTER * rng.standard_normal(4)
                    present[k, b, g] = lane["presence"][k, b, j] != 0 and rng.uniform() < 0.8
                box[k, b, N] = lane["box"][k, b, 0] + JITTER * rng.standard_normal(4)
                present[k, b, N] = lane["presence"][k, b, 0] != 0 and rng.uniform() < 0.5
        box[..., 2:] = np.maximum(box[..., 2:], 4.0)                       # (a box stays a box)
        truth.append(dict(box=box, present=present, valid=(rng.uniform(size=(Ts, B)) < 0.9).astype(np.int32)))
    return truth


def _truth(F, P, obs, noise, Ts=1):
    return unscored_truth(_stream(F, P, frames_per_step=Ts), obs, noise, Ts, cut=_cut)[0]


class _ScoreRef(object):
    """The score's reference carried along a stream, on the device's own matching (judged and imposed)."""

    def __init__(self):
        self.counts = self.iou_sum = self.last_id = None
        self.tol = 0.0
        self.judged = self.worst = 0

    def step(self, o, truth):
        lane = o["lane"]
        x = dict(box=lane["box"], presence=lane["presence"], obj_id=lane["obj_id"], map_count=lane["map_count"], truth_box=truth["box"],
                 truth_present=truth["present"], truth_valid=truth["valid"])
        err = R.iou32_error(truth["box"] * (truth["present"] != 0)[..., None], lane["box"])      # (over boxes that are boxes)
        on = (x["truth_valid"] != 0) & (x["map_count"] != -1)
        first = M.fragile_from(R.iou_table(x["truth_box"], x["box"]), x["truth_present"], x["presence"], on, IOU)
        assert (first == on.shape[0]).all(), "a candidate within 1e-5 of the threshold"
        judge = M.Judge([((t, b), lane["truth_match"][t, b]) for t, b in M.scored_frames(x)], M.slack(err * M.UNIT))
        with M.replaced(R, "assign", judge.assign):
            ref = R.score(iou_min=IOU, counts=self.counts, iou_sum=self.iou_sum, last_id=self.last_id, **x)
        assert judge.clean(), (judge.infeasible, judge.cardinality, judge.deficit)
        self.judged, self.worst = self.judged + judge.judged, max(self.worst, judge.worst_deficit)
        self.counts, self.iou_sum, self.last_id = ref.counts, ref.iou_sum, ref.last_id
        for n in _capi.SCORE_INT_FIELDS:
            assert np.array_equal(lane[n], getattr(ref, n)), (n, lane[n], getattr(ref, n))
        self.tol = max(self.tol, 4.0 * err)
        assert self.tol < 1e-5 and float(np.abs(lane["match_iou"].astype(np.float64) - ref.match_iou).max()) <= 4.0 * err

    def check(self, got):
        for i, n in enumerate(R.COUNTS):
            assert np.array_equal(got[n].numpy(), self.counts[:, i]), (n, got[n], self.counts[:, i])
        assert (np.abs(got["iou_sum"].numpy() - self.iou_sum) <= self.tol * self.counts[:, 3]).all()


def test_score_match_changes_only_the_score_and_equals_the_reference():
    F, P, obs, noise = _setup()
    truth = _truth(F, P, obs, noise)
    grd, opt, eager = _scored(F, P), _scored(F, P, score_match="optimal"), _scored(F, P, score_match="optimal", use_graph=False)
    ref, idf = _ScoreRef(), IdfRef()
    differ = more = 0
    for t in range(T):
        f = slice(t, t + 1)
        o, b, c = (host(s.step(obs[f], noise=noise[f], truth=truth[t])) for s in (grd, opt, eager))
        others = set(o["lane"]) - SCORE_KEYS
        assert set(o["lane"]) == set(b["lane"]) and IDENT_KEYS <= others
        same_bits(o, b, OUTS + SMC_OUTS, t)
        same_bits(o["lane"], b["lane"], others, t)                        # the estimate's and the identity's outputs: untouched
        same_bits(b["lane"], c["lane"], b["lane"].keys(), (t, "eager"))   # eager and graph: the same bits
        for k in STATE:
            assert torch.equal(getattr(grd, k), getattr(opt, k)), (t, k)
        ref.step(b, truth[t])
        idf.step(b, truth[t])
        scored = b["lane"]["tp"] >= 0
        assert np.array_equal(scored, o["lane"]["tp"] >= 0) and (b["lane"]["tp"] >= o["lane"]["tp"])[scored].all(), (t, b["lane"]["tp"], o["lane"]["tp"])
        differ += int(((b["lane"]["truth_match"] != o["lane"]["truth_match"]).any(-1) & scored).sum())
        more += int((b["lane"]["tp"] - o["lane"]["tp"])[scored].sum())
    assert opt.core.graph_nodes() == grd.core.graph_nodes()
    for k in grd._ident:
        assert torch.equal(grd._ident[k], opt._ident[k]), k
    got, got_eager, got_grd = opt.score(), eager.score(), grd.score()
    ref.check(got)
    assert all(torch.equal(got[n], got_eager[n]) for n in R.COUNTS + ("iou_sum",))
    for k in ("counts", "iou_sum", "last_id"):
        assert torch.equal(opt._score[k], eager._score[k]), k
    idf.check_table(opt)
    tot = idf.check_score(opt.idf_score())
    print("score_match: frames where the streams' matchings differ", differ, "pairs more", more, "judged", ref.judged, "worst deficit",
          ref.worst, "tp", int(got_grd["tp"].sum()), "->", int(got["tp"].sum()), "mota", got_grd["mota"], "->", got["mota"], tot)
    assert int(got["tp"].sum()) >= int(got_grd["tp"].sum()) and int(got["frames"].sum()) == int(got_grd["frames"].sum()) > 0
    for s in (grd, opt, eager):
        s.close()


def test_identity_match_changes_only_the_identity_and_equals_the_reference():
    F, P, obs, noise = _setup()
    truth = _truth(F, P, obs, noise)
    grd, opt, eager = _scored(F, P), _scored(F, P, identity_match="optimal"), _scored(F, P, identity_match="optimal", use_graph=False)
    outs = []
    for t in range(T):
        f = slice(t, t + 1)
        o, b, c = (host(s.step(obs[f], noise=noise[f], truth=truth[t])) for s in (grd, opt, eager))
        same_bits(o, b, OUTS + SMC_OUTS, t)
        same_bits(o["lane"], b["lane"], set(o["lane"]) - IDENT_KEYS, t)   # the score reads obj_id: it is untouched too
        same_bits(b["lane"], c["lane"], b["lane"].keys(), (t, "eager"))
        for k in STATE:
            assert torch.equal(getattr(grd, k), getattr(opt, k)), (t, k)
        outs.append(b["lane"])
    assert opt.core.graph_nodes() == grd.core.graph_nodes()
    for k in ("counts", "iou_sum", "last_id"):
        assert torch.equal(grd._score[k], opt._score[k]), k
    for k in grd._idf:
        assert torch.equal(grd._idf[k], opt._idf[k]), k
    for k in opt._ident:
        assert torch.equal(opt._ident[k], eager._ident[k]), k
    # the reference on the device's own links
    y = {n: np.concatenate([o[n] for o in outs]) for n in ("box", "presence", "obj_id", "what", "best_row")}
    how, lane_id, track_len = (np.concatenate([o[n] for o in outs]) for n in ("id_how", "lane_id", "track_len"))
    la = opt.lane
    kw = dict(iou_min=la.identity_iou, reid_dist=la.reid_dist, reid_what=la.reid_what, M=la.M, max_age=int(la.max_age), appearance=True)
    follower = M.IdentityFollower(B, N, y["what"].shape[-1], kw, R.iou32_error(y["box"][:-1], y["box"][1:]) * M.UNIT,
                                  I.measured_tol(y["box"], y["best_row"], y["what"], True))
    out = follower.feed(y, how, lane_id)
    whole, upto = follower.whole(), follower.upto()
    print("identity_match: judged", follower.judged, "of", follower.asked, "lanes compared to the end", int(whole.sum()), "of", B,
          "worst deficit", follower.worst)
    assert not follower.failures, follower.failures[:4]
    assert upto.sum() >= T * B // 2
    for n, dev in (("lane_id", lane_id), ("how", how), ("track_len", track_len)):
        assert np.array_equal(dev[upto], out[n][upto]), n
    got = opt.identities()
    for i, n in enumerate(I.COUNTS):
        assert np.array_equal(got[n].numpy()[whole], follower.mem["counts"][whole, i]), n
    assert np.array_equal(got["trk_id"].numpy()[whole], follower.mem["trk_id"][whole])
    for s in (grd, opt, eager):
        s.close()


def test_three_frames_per_step_graph_equals_eager_in_both_modes():
    F, P, obs, noise = _setup(seed=13)
    truth = _truth(F, P, obs, noise, Ts=3)
    kw = dict(frames_per_step=3, score_match="optimal", identity_match="optimal")
    grd, opt, eager = _scored(F, P, frames_per_step=3), _scored(F, P, **kw), _scored(F, P, use_graph=False, **kw)
    ref = _ScoreRef()
    for s in range(T // 3):
        f = slice(3 * s, 3 * s + 3)
        o, b, c = (host(st.step(obs[f], noise=noise[f], truth=truth[s])) for st in (grd, opt, eager))
        same_bits(o, b, OUTS + SMC_OUTS, s)
        same_bits(b["lane"], c["lane"], b["lane"].keys(), (s, "eager"))
        # (the identity's mode does not reach the score here: score_ids="row")
        ref.step(b, truth[s])
    assert opt.core.graph_nodes() == grd.core.graph_nodes()
    ref.check(opt.score())
    for k in opt._ident:
        assert torch.equal(opt._ident[k], eager._ident[k]), k
    for k in ("counts", "iou_sum", "last_id"):
        assert torch.equal(opt._score[k], eager._score[k]), k
    for st in (grd, opt, eager):
        st.close()


def test_the_forecast_links_by_keep_and_optimal():
    F, P, obs, noise = _setup()
    st = _stream(F, P)
    for t in range(6):
        st.step(obs[t:t + 1], noise=noise[t:t + 1])
    FH, S = 3, 2
    call = lambda **kw: host(st.forecast(FH, samples=S, lane=True, seed=3, **kw))
    lane = call()["lane"]
    rng = np.random.default_rng(3)
    a_box, a_present = np.zeros((B, G, 4), np.float32), np.zeros((B, G), np.int32)
    for g in range(G):      # every truth a coarse copy of object g % N: two truths on object 0
        a_box[:, g] = lane["box0"][:, g % N] + JITTER * rng.standard_normal((B, 4))
        a_present[:, g] = lane["presence"][:, g % N] != 0
    a_box[..., 2:] = np.maximum(a_box[..., 2:], 4.0)
    truth = dict(box=np.broadcast_to(a_box, (FH, B, G, 4)).copy(), present=np.broadcast_to(a_present, (FH, B, G)).copy(),
                 anchor_box=a_box, anchor_present=a_present)
    grd, opt = call(truth=truth), call(truth=truth, link_match="optimal")
    s_grd, s_opt = grd["lane"].pop("score"), opt["lane"].pop("score")
    same_bits(grd, opt, where="forecast.")                                      # everything but the score: the same bits
    tab = {n: lane[n] for n in _capi.TRAJ_TABLE_FIELDS if n in lane}
    tr = dict(anchor_box=a_box, anchor_present=a_present, anchor_valid=np.ones(B, np.int32), truth_box=truth["box"],
              truth_present=truth["present"], truth_valid=np.ones((FH, B), np.int32))
    iou = TR.anchor_iou(tab, tr)
    e = float(np.abs(TR.anchor_iou(tab, tr, np.float32).astype(np.float64) - iou).max())
    on = TR.lane_on(tab, tr)
    assert (M.fragile_from(iou[None], a_present[None], tab["presence"][None], on[None], IOU) == 1).all(), "a candidate within 1e-5"
    judge = M.Judge([(int(b), s_opt["link"][b]) for b in np.nonzero(on)[0]], M.slack(e * M.UNIT))
    with M.replaced(TR, "assign", judge.assign):
        ref = TR.score(tab, tr, IOU)
    assert judge.clean() and judge.judged == int(on.sum()), (judge.infeasible, judge.cardinality, judge.deficit)
    assert np.array_equal(s_opt["link"], ref.link) and np.array_equal(s_opt["state"], ref.state)
    assert np.array_equal(s_grd["link"], TR.score(tab, tr, IOU).link)
    # link_match joins the key of the accumulators: the optimal call started fresh ones, which hold that one call
    got = st.trajectory_score("forecast")
    assert int(got["calls"].sum()) == int(on.sum()) and np.array_equal(got["linked"].numpy(), ref.lane_counts[:, 3])
    print("forecast link: linked greedy", int((s_grd["link"] >= 0).sum()), "optimal", int((s_opt["link"] >= 0).sum()))
    assert (s_opt["link"] >= 0).sum() >= (s_grd["link"] >= 0).sum()
    with pytest.raises(ValueError, match="link_match='optimal' is for a call with truth"):
        st.forecast(FH, samples=S, lane=True, link_match="optimal")
    st.close()
