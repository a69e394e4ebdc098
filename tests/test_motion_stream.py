"""-m gpu: lane motion inside the streaming pass (include/sqair_hip.h: sqair_set_motion; SqairStream(estimate=True, identity=True,
motion=True)), B = 4, K = 5, N = 3, 50 x 50, two dozen frames of make_sequences.

Checked here: ``motion=False`` is the identity stream -- every output, the lane answer, the blob, the SMC accumulators, the track
table and the counters bit for bit --, and ``sqair_graph_nodes`` is the same with the motion on and off: the identity's node is replaced,
none is added.  With the motion on, everything that does not depend on ``lane_id`` is still the identity stream's bit for bit, alone
and composed with ``missing=True``, SMC and ``score_ids="lane"``; graph replay and eager steps give the same bits; ``out["lane"]``
gains ``velocity`` (and ``nis`` when asked for); the integer outputs, the table and ``identities()`` equal the float64 reference
(tests/motion_ref.py) run on the steps' own lane outputs, velocity, nis and the filter's state within the bar measured on that run;
stepping one frame at a time equals chunks of three, bit for bit; ``reset(lanes)`` frees the lanes' tracks."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import motion_ref as MR
from tests.stream_harness import EST_KEYS, OUTS, SMC_OUTS, SCORE, host, make_truth, run, same_bits, setup, stream, words

pytestmark = pytest.mark.gpu

ID_KEYS = {"lane_id", "id_how", "track_len"}
HW = (50, 50)
FLAGS = dict(k_particles=5, n_steps_per_image=3)
B, N, M = 4, 3, 6
CFG = dict(iou_min=0.3, reid_dist=4.0, reid_what=float("inf"), M=M, max_age=3)
SCALARS = (0.25, 1.0, 16.0, 3.0)
IDENT = dict(identity=True, identity_iou=CFG["iou_min"], identity_reid_dist=CFG["reid_dist"], identity_max_age=CFG["max_age"])
MOTION = dict(motion=True, motion_q=SCALARS[0], motion_r=SCALARS[1], motion_v0=SCALARS[2], motion_gate=SCALARS[3])
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)
CARRIED = ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src")
T = 24


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=0.5, **kw)


def _equal(a, b):
    return torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def _check(st, outs, resets=None):
    """The stream's identity and motion outputs, table and counters against the reference on the steps' own lane outputs."""
    lane = {k: np.concatenate([o["lane"][k] for o in outs]) for k in ("box", "presence", "obj_id", "what", "best_row")}
    Ts, frames = outs[0]["lane"]["best_row"].shape[0], lane["best_row"].shape[0]
    cuts = sorted(set([0, len(outs)] + list(resets or {})))
    mem, parts = None, []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if mem is not None and a in (resets or {}):
            mem["trk_id"][resets[a]] = -1
        parts.append(MR.identity(mem=mem, motion=SCALARS, **CFG, **{k: v[a * Ts:b * Ts] for k, v in lane.items()}))
        mem = parts[-1].mem
    err = {k: max(p.err[k] for p in parts) for k in ("iou", "d2", "dw")}
    err.update({k: np.max([p.err[k] for p in parts], 0) for k in ("velocity", "nis", "kf")})
    tol = MR.measured_tol(err)
    assert tol.iou < 1e-3 and tol.d2 < 1e-2 and tol.dw < 1e-4, tol
    first = MR.fragile_from(np.concatenate([p.margins for p in parts]), tol)
    whole = first == frames
    if not whole.all():
        print("lanes left out as fragile from frame:", {int(b): int(first[b]) for b in np.flatnonzero(~whole)})
    assert whole.sum() >= B - 1, "more than one fragile lane: a decisive compare inside the fp32 band"
    upto = np.arange(frames)[:, None] < first[None, :]
    got = {n: np.concatenate([o["lane"][n] for o in outs]) for n in ("lane_id", "id_how", "track_len", "velocity") + (("nis",) if "nis" in outs[0]["lane"] else ())}
    for n, w in (("lane_id", "lane_id"), ("id_how", "how"), ("track_len", "track_len")):
        want = np.concatenate([getattr(p, w) for p in parts])
        assert got[n].dtype == np.int32 and np.array_equal(got[n][upto], want[upto]), n
    bars = MR.bars(err, whole)
    vel, nis = np.concatenate([p.velocity for p in parts]), np.concatenate([p.nis for p in parts])
    assert got["velocity"].dtype == np.float32 and got["velocity"].shape == (frames, B, N, 2)
    assert np.abs(got["velocity"] - vel)[upto].max() <= bars["velocity"], (np.abs(got["velocity"] - vel)[upto].max(), bars)
    if "nis" in got:
        assert np.abs(got["nis"] - nis)[upto].max() <= bars["nis"], (np.abs(got["nis"] - nis)[upto].max(), bars)
    ids = st.identities()
    for i, n in enumerate(MR.COUNTS):
        assert np.array_equal(ids[n].numpy()[whole], mem["counts"][whole, i]), n
    live = (mem["trk_id"] >= 0) & whole[:, None]
    assert np.array_equal(ids["trk_id"].numpy()[whole], mem["trk_id"][whole])
    for n in ("trk_age", "trk_len", "trk_box"):
        assert np.array_equal(words(ids[n].numpy())[live], words(mem[n])[live]), n
    # the filter's state, by name, and what the host forms from it
    kf = mem["trk_kf"]
    assert set(ids) >= {"trk_centre", "trk_vel", "trk_sigma", "trk_pred_box"} and "trk_kf" not in ids
    for n, i in (("trk_centre", 0), ("trk_vel", 1)):
        assert ids[n].shape == (B, M, 2) and np.abs(ids[n].numpy() - kf[..., i])[live].max() <= bars["kf"], n
    dev = st._ident["trk_kf"].cpu()
    assert torch.equal(ids["trk_sigma"], dev[..., 2].sqrt()) and torch.equal(ids["trk_centre"], dev[..., 0])
    assert torch.equal(ids["trk_pred_box"], torch.cat([dev[..., 0] - 0.5 * ids["trk_box"][..., 2:], ids["trk_box"][..., 2:]], -1))
    tot = dict(zip(MR.COUNTS, mem["counts"][whole].sum(0).tolist()))
    assert tot["objects"] == tot["kept"] + tot["bridged"] + tot["reidentified"] + tot["born"] and tot["born"] > 0
    return tot


# ---- 1. off is the identity stream; on replaces the node; nothing that does not depend on lane_id moves --------------------------------
def test_motion_off_changes_nothing_and_on_replaces_the_node():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 11)
    ident, off = _stream(F, P, **SMC, **IDENT), _stream(F, P, motion=False, **SMC, **IDENT)
    on, eager = _stream(F, P, motion_nis=True, **SMC, **IDENT, **MOTION), _stream(F, P, use_graph=False, motion_nis=True, **SMC, **IDENT, **MOTION)
    outs = []
    for t in range(T):
        f = slice(t, t + 1)
        a, o, b, c = (host(s.step(obs[f], noise=noise[f])) for s in (ident, off, on, eager))
        assert set(o["lane"]) == EST_KEYS | ID_KEYS and set(b["lane"]) == EST_KEYS | ID_KEYS | {"velocity", "nis"}
        same_bits(a, o, None, (t, "off"))                                  # off: every output, the lane answer included
        same_bits(a, b, OUTS + SMC_OUTS, (t, "on"))                        # on: what does not depend on lane_id
        same_bits(a["lane"], b["lane"], EST_KEYS, (t, "on"))
        same_bits(b, c, None, (t, "eager"))                                # eager and graph: the same bits
        for k in CARRIED:
            assert torch.equal(getattr(ident, k), getattr(off, k)) and torch.equal(getattr(ident, k), getattr(on, k)), (t, k)
        assert b["lane"]["velocity"].shape == (1, B, N, 2) and b["lane"]["nis"].shape == (1, B, N)
        outs.append(b)
    assert set(ident._ident) == set(off._ident) and all(_equal(ident._ident[k], off._ident[k]) for k in ident._ident)
    assert all(_equal(on._ident[k], eager._ident[k]) for k in on._ident) and "trk_kf" in on._ident
    nodes = ident.core.graph_nodes()
    assert off.core.graph_nodes() == nodes and on.core.graph_nodes() == nodes      # replaced, not added
    tot = _check(on, outs)
    print("smc", tot, "nodes", nodes)
    assert not any(k in off.identities() for k in ("trk_centre", "trk_vel", "trk_sigma", "trk_pred_box"))
    for s in (ident, off, on, eager):
        s.close()


# ---- 2. one frame at a time equals chunks of three -----------------------------------------------------------------------------------------
def test_single_steps_equal_chunks_of_three():
    """Without SMC the two runs see the same rows; the kernel's five inputs are compared first (the estimate's weights may differ in
    the last bit between the two: the host adds a step's log weights to the carried sum in another order)."""
    F, P, obs, noise = setup(FLAGS, B, T, HW, 3)
    kw = dict(motion_nis=True, **IDENT, **MOTION)
    one, three = _stream(F, P, frames_per_step=1, **kw), _stream(F, P, frames_per_step=3, **kw)
    singles, chunks = run(one, obs, noise, 1), run(three, obs, noise, 3)
    for n in ("box", "presence", "obj_id", "what", "best_row") + tuple(sorted(ID_KEYS)) + ("velocity", "nis"):
        assert np.array_equal(words(np.concatenate([o["lane"][n] for o in chunks])), words(np.concatenate([o["lane"][n] for o in singles]))), n
    assert all(_equal(one._ident[k], three._ident[k]) for k in one._ident)
    print("T3", _check(three, chunks))
    one.close()
    three.close()


# ---- 3. reset ---------------------------------------------------------------------------------------------------------------------------
def test_reset_frees_the_lanes_tracks():
    F, P, obs, noise = setup(FLAGS, B, T, HW, 19)
    st = _stream(F, P, **IDENT, **MOTION)
    resets = {8: [1], 15: [0, 3]}

    def before(s):
        if s in resets:
            torch.cuda.synchronize()
            was = {k: v.clone() for k, v in st._ident.items()}
            st.reset(resets[s])
            torch.cuda.synchronize()
            lanes, keep = resets[s], [b for b in range(B) if b not in resets[s]]
            assert (st._ident["trk_id"][lanes] == -1).all() and torch.equal(st._ident["trk_id"][keep], was["trk_id"][keep])
            assert all(torch.equal(st._ident[k], was[k]) for k in was if k != "trk_id")      # the filter's state stays: never read
    outs = run(st, obs, noise, before=before)
    assert "nis" not in outs[0]["lane"] and "velocity" in outs[0]["lane"]                    # nis only when asked for
    print("reset", _check(st, outs, resets))
    ids = np.concatenate([o["lane"]["lane_id"] for o in outs])
    for s, lanes in resets.items():      # after a reset every id of the lane is a fresh one
        for b in lanes:
            assert not set(ids[:s, b][ids[:s, b] >= 0].tolist()) & set(ids[s:, b][ids[s:, b] >= 0].tolist()), (s, b)
    st.close()


# ---- 4. composed: missing frames, SMC, the score on lane ids ---------------------------------------------------------------------------
def test_composed_with_missing_smc_and_the_score_on_lane_ids():
    """What depends on lane_id: the identity's three outputs and, with score_ids="lane", whatever the score, the IDF and the HOTA
    derive from the id words (the keep step can move a match, so tp, fn, fp and idsw may differ too).  Everything before the identity
    is held to the same bits, the score's id-free counters and the clips' frame counts to the same values, the node count to the same
    number -- with identity_match="optimal", so the node replaced is k_lane_identity_opt."""
    F, P, obs, noise = setup(SCORE.FLAGS, SCORE.B, T, SCORE.HW, 11)
    rng = np.random.default_rng(2)
    observed = np.stack([np.ones(SCORE.B, bool) if t < 2 else rng.uniform(size=SCORE.B) < 0.7 for t in range(T)])
    mk = lambda **kw: stream((F, SCORE.HW, P), SCORE.B, outputs=OUTS, estimate=True, estimate_iou=0.5, missing=True, **SMC, **kw)
    plain = mk()
    truth = make_truth(run(plain, obs, noise, observed=observed), 1)
    plain.close()
    sc = dict(score=True, score_iou=SCORE.IOU, score_truth=SCORE.G, score_ids="lane", score_idf=True, score_hota=True, **IDENT)
    off, on = mk(**sc), mk(identity_match="optimal", **sc, **MOTION)
    ref = mk(identity_match="optimal", **sc)
    a, b, r = (run(s, obs, noise, observed=observed, truth=truth) for s in (off, on, ref))
    assert on.core.graph_nodes() == ref.core.graph_nodes() == off.core.graph_nodes()
    for x, y in zip(r, b):
        same_bits(x, y, OUTS + SMC_OUTS, "composed")
        same_bits(x["lane"], y["lane"], EST_KEYS, "composed")
    for k in CARRIED:
        assert torch.equal(getattr(ref, k), getattr(on, k)), k
    got, want = on.score(), ref.score()
    for n in ("frames", "frames_invalid", "truth", "count_hit", "count_abs_err"):             # (no id enters these)
        assert torch.equal(got[n], want[n]), n
    assert int(got["tp"].sum()) > 0 and on.idf_score()["frames"].sum() == ref.idf_score()["frames"].sum()
    assert on.hota_score()["frames"].sum() == ref.hota_score()["frames"].sum()
    ids = on.identities()
    assert int(ids["objects"].sum()) == int(ref.identities()["objects"].sum()) > 0
    vel = np.concatenate([o["lane"]["velocity"] for o in b])
    assert np.isfinite(vel).all() and (vel != 0).any()
    for s in (off, on, ref):
        s.close()


def test_call_errors():
    F, P, obs, noise = setup(FLAGS, B, 1, HW, 11)
    with pytest.raises(ValueError, match=r"^SqairStream: motion is for a stream with identity=True"):
        _stream(F, P, motion=True)
    st = _stream(F, P, **IDENT, **MOTION)
    assert st._ident["trk_kf"].shape == (B, 2 * N, 2, 5) and _capi.MOTION_MEMORY == ("trk_kf",)
    st.close()
