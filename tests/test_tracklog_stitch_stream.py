"""-m gpu: track log stitching on a stream (SqairStream(estimate=True, identity=True, tracklog=L); ``track_log(lag, stitch=True)``;
include/sqair_hip.h: sqair_lane_tracklog_stitch), B = 4, K = 3 or 5, N = 3, 50 x 50, a dozen frames of make_sequences, an identity
that forgets a track after one unseen frame, so that the log holds fragments.

Checked here: ``track_log(lag, stitch=True)`` equals the reference's stitch (tests/tracklog_stitch_ref.py) of the log rebuilt from the
steps' own outputs -- every integer exactly, ``d2`` within four times the reference's measured fp32 error, the stitched states within
the bars measured on that run --; ``stitch=False`` returns the bytes of a stream that never stitched, and the plain keys of a
``stitch=True`` result are those bytes; a stitch between steps changes no step output and no node count; ``reset([1])``,
``missing=True`` and SMC compose; with ``tracklog_truth=G`` and ``score=True`` the stitched table's score is the scorer's reference on
the stitched table read back."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.lane import mot_rows
from tests import tracklog_ref as R
from tests import tracklog_score_ref as SCR
from tests import tracklog_stitch_cases as SC
from tests import tracklog_stitch_ref as SR
from tests.stream_harness import OUTS, SCORE, make_truth, run, same_bits, same_bytes, setup, stream, words

pytestmark = pytest.mark.gpu

HW = (50, 50)
FLAGS = dict(k_particles=5, n_steps_per_image=3)
B, N, G, L, TRACKS = 4, 3, SCORE.G, 12, 8
IDENT = dict(identity=True, identity_iou=0.3, identity_reid_dist=4.0, identity_max_age=1)
SCALARS = (0.25, 1.0, 16.0)
LOG = dict(tracklog=L, tracklog_tracks=TRACKS)
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)
T = 12
GATE = 3.5
EXACT = ("track_id", "n_tracks", "len0", "frame_index", "state", "size")
PLAIN = EXACT + ("smooth", "filtered")
K = {n: i for i, n in enumerate(SCR.COUNTS)}


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=0.5, **kw)


def _reference_log(outs, resets=None):
    """The reference's append of the steps' own lane outputs; ``resets``: {step: lanes} whose count is zeroed ahead of that step."""
    log = R.new_log(B, L, N)
    for s, o in enumerate(outs):
        for b in (resets or {}).get(s, ()):
            log["count"][b] = 0
        lane = o["lane"]
        log = R.append(log, lane["lane_id"], lane["track_len"], lane["best_row"], lane["box"])
    return log


def _flat(log):
    out = {}
    for k, v in log.items():
        if isinstance(v, dict):
            out.update({k + "." + kk: vv for kk, vv in _flat(v).items()})
        else:
            out[k] = v.numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return out


def _check(st, outs, case, lag=L, max_gap=None, resets=None, **more):
    """track_log(lag, stitch=True) against the reference's stitch of the log rebuilt from the steps' outputs; returns both."""
    log = _reference_log(outs, resets)
    with np.errstate(all="ignore"):
        sm = R.smooth(log, lag, TRACKS, *SCALARS)
        ref = SR.stitch(log, sm, lag, TRACKS, *SCALARS, GATE, lag if max_gap is None else max_gap)
    assert ref.undecided == 0, "a candidate within the fp32 error of a decision: move the clip's seed"
    res = st.track_log(lag=lag, q=SCALARS[0], r=SCALARS[1], v0=SCALARS[2], stitch=True, stitch_gate=GATE, stitch_max_gap=max_gap, **more)
    got = res["stitched"]
    links = got["links"]
    assert set(links) == {"next", "d2", "gap", "root", "n_links"} and set(got) >= set(PLAIN) | {"links"}
    for name, want in (("next", ref.link_next), ("gap", ref.link_gap), ("root", ref.root), ("n_links", ref.n_links)):
        assert links[name].dtype == torch.int32 and np.array_equal(links[name].numpy(), want), (case, name, links[name], want)
    for k in EXACT:
        w = getattr(ref.table, k)
        assert got[k].numpy().dtype == w.dtype and np.array_equal(words(got[k].numpy()), words(w)), (case, k)
    d2_err = float(np.abs(links["d2"].numpy().astype(np.float64) - ref.link_d2).max())
    bars = R.bars(ref.table.err)
    errs = {}
    for name, states in (("filtered", ref.table.filt), ("smooth", ref.table.smooth)):
        d = got[name]
        errs[name] = max(float(np.abs(d["centre"].numpy() - states[..., 0]).max()), float(np.abs(d["velocity"].numpy() - states[..., 1]).max()))
    print(case, "links", ref.n_links.tolist(), "tracks", sm.n_tracks.tolist(), "->", ref.table.n_tracks.tolist(), "d2 error", d2_err,
          "allowed", 4.0 * ref.d2_err, "stitched errors", errs, "bars", bars)
    SC.record("stream", case, links=ref.n_links.tolist(), tracks=sm.n_tracks.tolist(), d2=dict(kernel_error=d2_err, allowed=4.0 * ref.d2_err),
              bars=bars, kernel_error=errs)
    assert d2_err <= 4.0 * ref.d2_err and errs["filtered"] <= bars["filt"] and errs["smooth"] <= bars["smooth"], (d2_err, errs, bars)
    return res, ref


# ---- 1. the stitch is the reference's; without it nothing changes ----------------------------------------------------------------------
def test_the_stitch_is_the_references_and_changes_nothing_else():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 11)
    never, on = _stream(F, P, **IDENT, **LOG), _stream(F, P, **IDENT, **LOG)
    kw = dict(q=SCALARS[0], r=SCALARS[1], v0=SCALARS[2])

    def before(s):
        if s in (5, 9):
            on.track_log(stitch=True, **kw)                                   # a stitch between steps
    a, b = run(never, obs, noise), run(on, obs, noise, before=before)
    for t, (x, y) in enumerate(zip(a, b)):
        same_bits(x, y, None, (t, "a stitch between steps"))
    assert on.core.graph_nodes() == never.core.graph_nodes()                  # no node is added
    for n in _capi.TRACKLOG_FIELDS:
        assert torch.equal(never._tracklog[n].view(torch.uint8), on._tracklog[n].view(torch.uint8)), n
    want = _flat(never.track_log(**kw))
    assert not any(k.startswith("stitched") for k in want)
    res, ref = _check(on, b, "single_steps")
    assert int(ref.n_links.sum()) > 0, "the clip holds no fragments to stitch: move its seed"
    same_bytes({k: v for k, v in _flat(res).items() if not k.startswith("stitched.")}, want, None, "the plain keys of a stitch=True result")
    same_bytes(_flat(on.track_log(**kw)), want, None, "stitch=False after a stitch")
    for b_ in range(B):                                                       # the exporter reads the stitched table unchanged
        rows = mot_rows(res["stitched"], b_)
        assert rows.shape[1] == 6 and len(rows) >= len(mot_rows(res, b_)) and set(rows[:, 1]) <= set(res["track_id"][b_].tolist())
    _check(on, b, "lag_7_gap_2", lag=7, max_gap=2)
    for s in (never, on):
        s.close()


# ---- 2. composed: reset, missing frames, SMC ---------------------------------------------------------------------------------------------
def test_reset_missing_and_smc_compose():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 19)
    rng = np.random.default_rng(2)
    observed = np.stack([np.ones(B, bool) if t < 2 else rng.uniform(size=B) < 0.7 for t in range(T)])
    st = _stream(F, P, missing=True, **SMC, **IDENT, **LOG)

    def before(s):
        if s == 7:
            st.reset([1])
    outs = run(st, obs, noise, before=before, observed=observed)
    res, ref = _check(st, outs, "reset_missing_smc", resets={7: [1]})
    assert res["stitched"]["frame_index"][:, 1].tolist() == [-1] * (L - (T - 7)) + list(range(T - 7))
    st.close()


# ---- 3. the stitched table scored ----------------------------------------------------------------------------------------------------------
def test_the_stitched_tables_score_is_the_scorers_reference_on_it():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 11)
    plain = _stream(F, P, **IDENT)
    truth = make_truth(run(plain, obs, noise), 1)
    plain.close()
    st = _stream(F, P, tracklog_truth=G, **IDENT, **LOG)
    outs = run(st, obs, noise, truth=truth)
    res, ref = _check(st, outs, "scored", score=True, score_iou=0.5)
    torch.cuda.synchronize()
    window = dict(truth_box=np.stack([t["box"][0] for t in truth]), truth_present=np.stack([t["present"][0] for t in truth]).astype(np.int32),
                  truth_valid=np.stack([t["valid"][0] for t in truth]).astype(np.int32))      # (T == L: the window is the clip)
    log_valid = st._tracklog["log_valid"].cpu().numpy()
    for key, dev in (("score", st.lane._log_out["out"]), ("stitched", st.lane._log_out["stitch"]["out"])):
        table = {k: dev[k].cpu().numpy() for k in SCR.TABLE}
        want = SCR.score(table, log_valid, window, 0.5)
        sc = res["score"] if key == "score" else res["stitched"]["score"]
        assert tuple(sc) == SCR.VIEWS
        for v, name in enumerate(SCR.VIEWS):
            for n in SCR.COUNTS:
                assert sc[name][n].tolist() == want.counts[:, v, K[n]].tolist(), (key, name, n)
        print(key, "smooth_filled", dict(zip(SCR.COUNTS, want.counts.sum(0)[3].tolist())))
    st.close()
