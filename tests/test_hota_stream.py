"""-m gpu: HOTA scoring inside the streaming pass (include/sqair_hip.h: sqair_set_hota; SqairStream(estimate=True, score=True,
score_hota=True)): B = 4, K = 5, N = 3, 50 x 50, SMC, identity=True with score_ids="lane", twelve steps.

The truth is made from an untruthed run's own lane answers the way tests/test_score_stream.py makes its truth (tests/stream_harness.py: make_truth) (shifted, rotated
between the slots every four frames, thinned, some added), so that matches, misses and id changes all occur.  Checked here: the log
equals the reference's append (tests/hota_ref.py) on the returned lane answers -- columns, rows and counters exactly, q within +-1
--; ``hota_score()`` equals the reference's solve of the stream's own log on the device's own matching, which is judged; every other
output of the stream is bit-identical with and without ``score_hota``, with and without ``score_idf``, and the graph has exactly one
node more; graph replay and eager steps leave the same log; one frame per step and four (no resampling in between, so that the rows
are the same) give the same tables; ``reset(lanes)`` closes those lanes' clips; ``hota_score(reset=True)`` restarts the totals."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.lane import hota_figures
from tests import hota_ref as R
from tests.hota_cases import RTOL
from tests.stream_harness import OUTS, SCORE, SMC_OUTS, host, same_bits, setup, stream, unscored_truth

pytestmark = pytest.mark.gpu

HW, B, G, N, IOU = SCORE.HW, SCORE.B, SCORE.G, SCORE.N, SCORE.IOU
FLAGS = dict(k_particles=5, n_steps_per_image=N)
P_IDS, L_FRAMES = 6, 8
T = 12
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)
SUMS = tuple(n + "_sum" for n in R.FLOAT)      # hota_score()'s names of the three double sums
CARRIED = ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src")


def _setup(seed=11):
    return setup(FLAGS, B, T, HW, seed)


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=IOU, identity=True, **dict(SMC, **kw))


def _scored(F, P, hota=True, **kw):
    more = dict(score_hota=True, score_hota_ids=P_IDS, score_hota_frames=L_FRAMES) if hota else {}
    return _stream(F, P, score=True, score_iou=IOU, score_truth=G, score_ids="lane", **dict(more, **kw))


def _truth(F, P, obs, noise, **kw):
    return unscored_truth(_stream(F, P, **kw), obs, noise)[0]


def _log(st):
    torch.cuda.synchronize()
    return {n: st._hota[n].cpu().numpy() for n in R.LOG + R.TOTALS}


class _Ref(object):
    """The reference carried along a stream: the log, fed every step's own lane outputs (the id words are lane_id's)."""

    def __init__(self):
        self.log = R.new_log(B, G, N, P_IDS, L_FRAMES)

    def step(self, o, truth):
        lane = o["lane"]
        self.log = R.append(self.log, lane["box"], lane["presence"], lane["lane_id"], lane["map_count"], truth["box"], truth["present"],
                            truth["valid"])

    def close(self, lanes, st, log):
        """Closes the lanes' clips in ``log``, the stream's own log as it was before its reset (check_log has just held it to this
        reference's), on the device's matching."""
        mask = np.zeros(B, np.int32)
        mask[lanes] = 1
        self.log = _solved(st, log, close=mask)[0]

    def check_log(self, st):
        got = _log(st)
        for n in ("col_id", "frames", "dropped_frames", "totals_c"):
            assert np.array_equal(got[n], self.log[n]), (n, got[n], self.log[n])
        used = np.arange(L_FRAMES)[None, :] < got["frames"][:, None]      # (the records not in use are never read)
        for n in ("log_col", "log_row"):
            assert np.array_equal(got[n][used], self.log[n][used]), (n, got[n], self.log[n])
        a, b = got["log_q"][used].astype(np.int64), self.log["log_q"][used].astype(np.int64)
        assert np.array_equal(a < 0, b < 0) and np.abs(a - b).max() <= 1, np.abs(a - b).max()
        return got


def _solved(st, log, close=None):
    """The reference's solve of ``log`` (the stream's own) on the device's own matching: one more launch of the solve with ``match``
    bound, on a copy of the log, judged record by record and imposed."""
    core = st.core
    d = {n: torch.from_numpy(np.array(v)).cuda() for n, v in log.items()}
    d["work"] = torch.zeros_like(st._hota["work"])
    match = torch.full((B, L_FRAMES, G), -7, dtype=torch.int32, device="cuda")
    c = _capi.SqairLaneHota(P=P_IDS, L=L_FRAMES, **{n: d[n].data_ptr() for n in _capi.HOTA_LOG + _capi.HOTA_TOTALS})
    rc = core.lib.sqair_lane_hota_solve(core.handle, C.byref(c), G, N, B, None, None, None, None, match.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    match = match.cpu().numpy()
    tables = R.solve(log)[5]
    for b in range(B):
        for r in range(int(log["frames"][b])):
            R.judge(tables[b][r], match[b, r])
    return R.solve(log, close=close, match=match)[:4]


def _check_score(st, got, log):
    _, oi, of, oc = _solved(st, log)
    ints, floats, clip = log["totals_i"] + oi, log["totals_f"] + of, log["totals_c"] + oc
    for i, n in enumerate(R.INT):
        assert got[n].dtype == torch.int64 and np.array_equal(got[n].numpy(), ints[:, :, i]), n
    for i, n in enumerate(SUMS):
        assert got[n].dtype == torch.float64 and np.allclose(got[n].numpy(), floats[:, :, i], rtol=RTOL, atol=0.0), n
    for i, n in enumerate(R.CLIP):
        assert np.array_equal(got[n].numpy(), clip[:, i]), n
    same = lambda a, b: np.allclose(a, b, rtol=1e-11, atol=0.0, equal_nan=True)
    for want, have in [(R.figures(ints.sum(0), floats.sum(0)), got)] + [(R.figures(ints[b], floats[b]), got["lanes"][b]) for b in range(B)]:
        for n, v in want.items():
            assert same(have[n], v), (n, have[n], v)
    assert got["exact"] == (not clip[:, 2:].any())
    return dict(tp=ints[:, :, 0].sum(0).tolist(), fn=ints[:, 9, 1].sum(), fp=ints[:, 9, 2].sum(), clip=clip.sum(0).tolist())


def test_hota_changes_nothing_else_and_equals_the_reference():
    F, P, obs, noise = _setup()
    truth = _truth(F, P, obs, noise)
    off, on, eager = _scored(F, P, hota=False), _scored(F, P), _scored(F, P, use_graph=False)
    off_idf, on_idf = _scored(F, P, hota=False, score_idf=True, score_idf_ids=P_IDS), _scored(F, P, score_idf=True, score_idf_ids=P_IDS)
    streams = (off, on, eager, off_idf, on_idf)
    ref = _Ref()
    with pytest.raises(ValueError, match="keeps no HOTA log"):
        off.hota_score()
    for t in range(T):
        f = slice(t, t + 1)
        if t == 7:      # lanes 1 and 3 start a new clip
            before = ref.check_log(on)
            for s in streams:
                s.reset([1, 3])
            ref.close([1, 3], on, before)
            after = _log(on)
            keep = [0, 2]
            assert all(np.array_equal(before[n][keep], after[n][keep]) for n in before)
            assert (after["col_id"][[1, 3]] == -1).all() and not after["frames"][[1, 3]].any() and not after["dropped_frames"][[1, 3]].any()
            assert (after["totals_c"][[1, 3], 0] == 1).all() and np.array_equal(after["totals_c"][[1, 3], 1], before["frames"][[1, 3]])
            assert np.array_equal(after["totals_i"], ref.log["totals_i"]) and np.allclose(after["totals_f"], ref.log["totals_f"], rtol=RTOL, atol=0)
            ref.log["totals_f"] = after["totals_f"]      # (within the doubles' tolerance: the rest is compared against the device's own sums)
        o, b, c, oi, bi = (host(s.step(obs[f], noise=noise[f], truth=truth[t])) for s in streams)
        for x, y, sx, sy in ((o, b, off, on), (oi, bi, off_idf, on_idf)):
            assert set(x["lane"]) == set(y["lane"])      # nothing per frame: HOTA is not a per-frame quantity
            same_bits(x, y, OUTS + SMC_OUTS, t)
            same_bits(x["lane"], y["lane"], x["lane"].keys(), t)
            for k in CARRIED:
                assert torch.equal(getattr(sx, k), getattr(sy, k)), (t, k)
        same_bits(b["lane"], c["lane"], b["lane"].keys(), (t, "eager"))
        ref.step(b, truth[t])
    for sx, sy in ((off, on), (off_idf, on_idf)):
        for k in ("counts", "iou_sum", "last_id"):
            assert torch.equal(sx._score[k], sy._score[k]), k
        for k in sx._ident:
            assert torch.equal(sx._ident[k], sy._ident[k]), k
        assert sy.core.graph_nodes() == sx.core.graph_nodes() + 1
    for k in off_idf._idf:
        assert torch.equal(off_idf._idf[k], on_idf._idf[k]), k
    log = ref.check_log(on)
    for n, v in _log(eager).items():      # eager and graph: the same log
        assert np.array_equal(v, log[n]), n
    for n, v in _log(on_idf).items():
        assert np.array_equal(v, log[n]), n
    got = on.hota_score()
    seen = _check_score(on, got, log)
    assert all(np.array_equal(v, log[n]) for n, v in _log(on).items())      # reading the score closes nothing
    got_eager = eager.hota_score()
    assert all(torch.equal(got[n], got_eager[n]) for n in R.INT + SUMS + R.CLIP) and got["hota"] == got_eager["hota"]
    print(seen, {n: got[n] for n in ("hota", "deta", "assa", "loca", "hota0", "exact")})
    assert seen["clip"][0] == B + 2 and seen["tp"][0] > 0 and seen["fn"] > 0 and seen["fp"] > 0 and seen["tp"][0] > seen["tp"][-1]
    assert seen["clip"][2] > 0 and not got["exact"]      # L = 8 and twelve steps: the lanes that were not reset dropped frames
    # reset=True: the totals from zero, every log free
    on.hota_score(reset=True)
    again = on.hota_score()
    assert all(not again[n].any() for n in R.INT + SUMS + R.CLIP) and np.isnan(again["hota"]) and (on._hota["col_id"] == -1).all()
    for s in streams:
        s.close()


def test_one_frame_per_step_and_four_give_the_same_tables():
    """A pass resamples once, after its last frame, so that four frames per step carry other rows than one frame per step does
    unless no lane resamples: ess_frac is set below 1 / K here, which an ESS never falls under."""
    F, P, obs, noise = _setup(seed=13)
    never = dict(ess_frac=0.1)
    truth = _truth(F, P, obs, noise, **never)
    one, four = _scored(F, P, **never), _scored(F, P, frames_per_step=4, **never)
    ref = _Ref()
    for t in range(T):
        ref.step(host(one.step(obs[t:t + 1], noise=noise[t:t + 1], truth=truth[t])), truth[t])
    for s in range(T // 4):
        f = slice(4 * s, 4 * s + 4)
        four.step(obs[f], noise=noise[f], truth={k: np.concatenate([truth[t][k] for t in range(4 * s, 4 * s + 4)]) for k in truth[0]})
    assert not one.resampled.any()
    log = ref.check_log(one)
    for n, v in _log(four).items():
        assert np.array_equal(v, log[n]), n
    a, b = one.hota_score(), four.hota_score()
    assert all(torch.equal(a[n], b[n]) for n in R.INT + SUMS + R.CLIP)
    _check_score(one, a, log)
    assert np.isnan(hota_figures(np.zeros((19, 4)), np.zeros((19, 3)))["hota"])      # no denominator
    one.close()
    four.close()
