"""-m gpu: lane identities inside the streaming pass (include/sqair_hip.h: sqair_set_identity; SqairStream(estimate=True,
identity=True)), B = 4, K = 5, N = 3, 50 x 50, two dozen frames of make_sequences.

Checked here: ``lane_id``, ``id_how`` and ``track_len`` of ``out["lane"]``, the track table and ``identities()`` equal the float64
reference (tests/identity_ref.py) run on the steps' own lane outputs -- all integers, compared exactly; a lane is left out from its first
fragile frame on (the band measured on the run's own boxes and what vectors), at most one of the four --; switching the identity on changes
nothing else, bit for bit (outputs, lane answer, state blob, SMC accumulators), and adds exactly one graph node; graph replay and eager
steps give the same bits; three frames per step equal three single steps; with SMC; with a coasted lane; ``reset()`` frees the lanes'
tracks and keeps ``next_id``; with ``score_ids="lane"`` the score equals the score's reference fed ``lane_id``, and its ``idsw`` is no
larger than with ``score_ids="row"`` on the same run.  Which of kept, bridged, re-identified, born and ended occurred is printed and each
is asserted against the reference's count; that all five are exercised is tests/test_identity_kernel.py's to guarantee."""
import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import identity_ref as IR
from tests import score_ref as SR
from tests.stream_harness import EST_KEYS, OUTS, SMC_OUTS, host, run, same_bits, setup, stream, words

pytestmark = pytest.mark.gpu

ID_KEYS = {"lane_id", "id_how", "track_len"}
HW = (50, 50)
FLAGS = dict(k_particles=5, n_steps_per_image=3)
B, N, G, M = 4, 3, 4, 6
CFG = dict(iou_min=0.3, reid_dist=4.0, reid_what=float("inf"), M=M, max_age=3)
IDENT = dict(identity=True, identity_iou=CFG["iou_min"], identity_reid_dist=CFG["reid_dist"], identity_max_age=CFG["max_age"])
SMC = dict(resample="systematic", ess_frac=0.5, seed=5)
# The score test's gates.  Its truth is cut from the lane's own boxes, and under random parameters those move arbitrarily far between
# two frames while the row keeps the object's obj_id: with the motion gates above, every such jump would be a new track by design.  What
# that test compares is the identity logic -- the same lineage first, then the nearest appearance -- so the gates are opened to the
# whole frame: any overlap links, any distance inside the frame re-identifies.  The gates themselves are tests/test_identity_kernel.py's.
OPEN = dict(CFG, iou_min=1e-3, reid_dist=100.0)
IDENT_OPEN = dict(IDENT, identity_iou=OPEN["iou_min"], identity_reid_dist=OPEN["reid_dist"])
T = 24


def _setup(T=T, seed=11):
    return setup(FLAGS, B, T, HW, seed)


def _stream(F, P, **kw):
    return stream((F, HW, P), B, outputs=OUTS, estimate=True, estimate_iou=0.5, **kw)


def _reference(outs, resets=None, appearance=True, cfg=CFG):
    """The reference over the whole run from the steps' own lane outputs; ``resets``: {step index: lanes freed before it}.  Returns
    the per-frame outputs concatenated, the final memory and per lane its first fragile frame (the run's length where none is): a lane
    is compared up to there, as in tests/test_identity_kernel.py, and at most one of the four lanes may be left out."""
    lane = {k: np.concatenate([o["lane"][k] for o in outs]) for k in ("box", "presence", "obj_id", "what", "best_row")}
    tol = IR.measured_tol(lane["box"], lane["best_row"], lane["what"], appearance)
    # (the bands only have to be small next to what they are compared with -- iou_min = 0.3, r * r >= 16, what vectors that differ by
    #  O(1); a model's boxes can be a few pixels wide, where the overlap's cancellation costs the fp32 IoU a few digits)
    assert tol.iou < 1e-3 and tol.dc2 < 1e-2 and tol.dw < 1e-4, tol
    Ts = outs[0]["lane"]["best_row"].shape[0]
    cuts = sorted(set([0, len(outs)] + list(resets or {})))
    mem, parts, first = None, [], np.full(B, len(outs) * Ts, np.int64)
    for a, b in zip(cuts[:-1], cuts[1:]):
        if mem is not None and a in (resets or {}):
            mem["trk_id"][resets[a]] = -1
        r = IR.identity(mem=mem, appearance=appearance, tol=tol, **cfg, **{k: v[a * Ts:b * Ts] for k, v in lane.items()})
        hit = (r.fragile_from < (b - a) * Ts) & (first == len(outs) * Ts)
        first[hit] = a * Ts + r.fragile_from[hit]
        mem = r.mem
        parts.append(r)
    whole = first == len(outs) * Ts
    if not whole.all():
        print("lanes left out as fragile from frame:", {int(b): int(first[b]) for b in np.flatnonzero(~whole)})
    assert whole.sum() >= B - 1, "more than one fragile lane: a decisive compare inside the fp32 band"
    return {n: np.concatenate([getattr(r, n) for r in parts]) for n in ("lane_id", "how", "track_len")}, mem, first


def _check(st, outs, resets=None, appearance=True, cfg=CFG):
    """The stream's identity outputs, table and counters against the reference; returns the events counted."""
    want, mem, first = _reference(outs, resets, appearance, cfg)
    got = {n: np.concatenate([o["lane"][_capi.IDENT_LANE_NAMES[n]] for o in outs]) for n in _capi.IDENT_FIELDS}
    upto = np.arange(got["lane_id"].shape[0])[:, None] < first[None, :]      # [frames, B]: before a lane's first fragile frame
    whole = first == got["lane_id"].shape[0]
    for n in _capi.IDENT_FIELDS:
        assert got[n].dtype == np.int32 and got[n].shape == want[n].shape and np.array_equal(got[n][upto], want[n][upto]), n
    ids = st.identities()
    for i, n in enumerate(IR.COUNTS):
        assert ids[n].dtype == torch.int64 and np.array_equal(ids[n].numpy()[whole], mem["counts"][whole, i]), (n, ids[n], mem["counts"][:, i])
    assert np.array_equal(ids["trk_id"].numpy()[whole], mem["trk_id"][whole]) and np.array_equal(ids["next_id"].numpy()[whole], mem["next_id"][whole])
    live = (mem["trk_id"] >= 0) & whole[:, None]
    for n in ("trk_age", "trk_len", "trk_box"):
        assert np.array_equal(words(ids[n].numpy())[live], words(mem[n])[live]), n
    torch.cuda.synchronize()
    dev = {n: st._ident[n].cpu().numpy() for n in st._ident}
    assert np.array_equal(dev["trk_word"][live], mem["trk_word"][live])
    assert ("trk_what" in dev) == appearance and (not appearance or np.array_equal(words(dev["trk_what"])[live], words(mem["trk_what"])[live]))
    tot = dict(zip(IR.COUNTS, mem["counts"][whole].sum(0).tolist()))
    pooled = lambda n: float(ids[n].sum()) / float(ids["objects"].sum())      # (the stream pools its own counters, over every lane)
    assert ids["bridged_rate"] == pytest.approx(pooled("bridged")) and ids["reidentified_rate"] == pytest.approx(pooled("reidentified"))
    assert tot["objects"] == tot["kept"] + tot["bridged"] + tot["reidentified"] + tot["born"] and tot["objects"] > 0 and tot["born"] > 0
    return tot


# ---- 1. nothing else changes; one node more; graph == eager; against the reference, with SMC -------------------------------------------
def test_the_identity_changes_nothing_else_and_equals_the_reference():
    F, P, obs, noise = _setup()
    off, on, eager = _stream(F, P, **SMC), _stream(F, P, **SMC, **IDENT), _stream(F, P, use_graph=False, **SMC, **IDENT)
    outs, went = [], 0
    for t in range(T):
        f = slice(t, t + 1)
        o, b, c = (host(s.step(obs[f], noise=noise[f])) for s in (off, on, eager))
        assert set(o["lane"]) == EST_KEYS and set(b["lane"]) == EST_KEYS | ID_KEYS
        same_bits(o, b, OUTS + SMC_OUTS, t)
        same_bits(o["lane"], b["lane"], EST_KEYS, t)
        for k in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src"):
            assert torch.equal(getattr(off, k), getattr(on, k)), (t, k)
        same_bits(b["lane"], c["lane"], b["lane"].keys(), (t, "eager"))      # eager and graph: the same bits
        assert all(b["lane"][n].shape == (1, B, N) and b["lane"][n].dtype == np.int32 for n in ID_KEYS)
        outs.append(b)
        went += int(b["resampled"].sum())
    assert went > 0
    assert on.core.graph_nodes() == off.core.graph_nodes() + 1
    tot = _check(on, outs)
    for k in on._ident:
        a, e = on._ident[k], eager._ident[k]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, e.view(torch.int32) if e.dtype == torch.float32 else e), k
    print("smc", tot, "occurred:", [n for n in ("kept", "bridged", "reidentified", "born", "ended") if tot[n] > 0])
    for s in (off, on, eager):
        s.close()


# ---- 2. without SMC; three frames per step; without appearance -----------------------------------------------------------------------------
@pytest.mark.parametrize("resample,Ts,appearance", [(None, 1, True), (None, 3, True), ("systematic", 3, True), (None, 1, False)],
                         ids=["plain", "plain_T3", "smc_T3", "plain_nowhat"])
def test_identity_against_reference(resample, Ts, appearance):
    F, P, obs, noise = _setup(seed=3)
    kw = dict(resample=resample, ess_frac=0.5, seed=17, identity_appearance=appearance, **IDENT)
    st = _stream(F, P, frames_per_step=Ts, **kw)
    outs = run(st, obs, noise, Ts)
    tot = _check(st, outs, appearance=appearance)
    print(resample, Ts, appearance, tot, "occurred:", [n for n in ("kept", "bridged", "reidentified", "born", "ended") if tot[n] > 0])
    if Ts == 3 and resample is None:      # three frames per step equal three single steps: the outputs and the whole memory
        # (without SMC the two runs see the same rows; the kernel's five inputs are compared first -- the estimate's weights may differ
        #  in the last bit between the two, the host adds a step's log weights to the carried sum in another order)
        one = _stream(F, P, frames_per_step=1, **kw)
        singles = run(one, obs, noise, 1)
        for n in ("box", "presence", "obj_id", "what", "best_row") + tuple(sorted(ID_KEYS)):
            assert np.array_equal(words(np.concatenate([o["lane"][n] for o in outs])), words(np.concatenate([o["lane"][n] for o in singles]))), n
        for k in st._ident:
            a, e = st._ident[k], one._ident[k]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, e.view(torch.int32) if e.dtype == torch.float32 else e), k
        one.close()
    st.close()


# ---- 3. a coasted lane needs no case of its own ------------------------------------------------------------------------------------------
def test_a_coasted_lane_needs_no_case_of_its_own():
    F, P, obs, noise = _setup(seed=13)
    rng = np.random.default_rng(2)
    observed = np.stack([np.ones(B, bool) if t < 2 else rng.uniform(size=B) < 0.6 for t in range(T)])
    st = _stream(F, P, missing=True, **IDENT)
    outs = run(st, obs, noise, observed=observed)
    tot = _check(st, outs)
    coasted = sum(int(((o["lane"]["lane_id"][0] >= 0).any(-1) & ~observed[t]).sum()) for t, o in enumerate(outs))
    print("coasted", tot, "coasted (frame, lane)s with an identified object:", coasted)
    assert coasted > 4
    st.close()


# ---- 4. reset ------------------------------------------------------------------------------------------------------------------------
def test_reset_frees_the_lanes_tracks_and_keeps_next_id():
    F, P, obs, noise = _setup(seed=19)
    st = _stream(F, P, **IDENT)
    resets = {8: [1], 15: [0, 3]}
    seen = {}

    def before(s):
        if s in resets:
            torch.cuda.synchronize()
            was = {k: v.clone() for k, v in st._ident.items()}
            st.reset(resets[s])
            torch.cuda.synchronize()
            lanes, keep = resets[s], [b for b in range(B) if b not in resets[s]]
            assert (st._ident["trk_id"][lanes] == -1).all() and torch.equal(st._ident["trk_id"][keep], was["trk_id"][keep])
            assert all(torch.equal(st._ident[k], was[k]) for k in was if k != "trk_id")      # next_id and the counters stay
            seen[s] = int(was["next_id"][lanes].min())
    outs = run(st, obs, noise, before=before)
    tot = _check(st, outs, resets)
    ids = np.concatenate([o["lane"]["lane_id"] for o in outs])
    for s, lanes in resets.items():      # after a reset every id of the lane is a fresh one: never reused
        for b in lanes:
            old, new = ids[:s, b][ids[:s, b] >= 0], ids[s:, b][ids[s:, b] >= 0]
            assert not set(old.tolist()) & set(new.tolist()), (s, b)
    assert min(seen.values()) > 0
    print("reset", tot)
    st.close()


# ---- 5. the score on lane ids ------------------------------------------------------------------------------------------------------------
def _make_truth(outs, seed=7):
    """One ``truth`` dict per step from an unscored run's lane boxes: jittered by 1.5 px, every object in the truth slot of its index (the
    truth's identity does not change), a fifth dropped, a stranger in the spare slot in a third of the frames."""
    rng = np.random.default_rng(seed)
    truth = []
    for o in outs:
        lane = o["lane"]
        box, present = np.zeros((1, B, G, 4), np.float32), np.zeros((1, B, G), np.int32)
        for b in range(B):
            for j in range(N):
                box[0, b, j] = lane["box"][0, b, j] + 1.5 * rng.standard_normal(4)
                present[0, b, j] = lane["presence"][0, b, j] != 0 and rng.uniform() < 0.8
            if rng.uniform() < 0.33:
                box[0, b, N], present[0, b, N] = (rng.uniform(0, 30), rng.uniform(0, 30), 12.0, 12.0), 1
        truth.append(dict(box=box, present=present, valid=(rng.uniform(size=(1, B)) < 0.9).astype(np.int32)))
    return truth


def _score_reference(outs, truth, ids_of):
    counts = iou_sum = last_id = None
    for o, tr in zip(outs, truth):
        lane = o["lane"]
        ref = SR.score(box=lane["box"], presence=lane["presence"], obj_id=ids_of(lane), map_count=lane["map_count"], truth_box=tr["box"],
                       truth_present=tr["present"], truth_valid=tr["valid"], iou_min=0.5, counts=counts, iou_sum=iou_sum, last_id=last_id)
        first = SR.fragile_from(ref.iou, lane["presence"], lane["map_count"], tr["present"], tr["valid"], 0.5)
        assert (first == 1).all(), "a fragile frame of the score"
        for n in _capi.SCORE_INT_FIELDS:
            assert np.array_equal(lane[n], getattr(ref, n)), n
        counts, iou_sum, last_id = ref.counts, ref.iou_sum, ref.last_id
    return counts, last_id


def test_the_score_on_lane_ids_equals_its_reference_and_switches_no_more_often():
    F, P, obs, noise = _setup()
    plain = _stream(F, P, **SMC)
    truth = _make_truth(run(plain, obs, noise))
    plain.close()
    sc = dict(score=True, score_iou=0.5, score_truth=G, **SMC, **IDENT_OPEN)
    row, lane = _stream(F, P, score_ids="row", **sc), _stream(F, P, score_ids="lane", **sc)
    a, b = run(row, obs, noise, truth=truth), run(lane, obs, noise, truth=truth)
    assert lane.core.graph_nodes() == row.core.graph_nodes()                   # the same launches: only a pointer differs
    for x, y in zip(a, b):
        same_bits(x["lane"], y["lane"], EST_KEYS | ID_KEYS, "score_ids")
    counts_row, _ = _score_reference(a, truth, lambda l: l["obj_id"])
    counts_lane, last = _score_reference(b, truth, lambda l: l["lane_id"].view(np.float32))   # (the score takes the id as a 32-bit word)
    got_row, got_lane = row.score(), lane.score()
    for i, n in enumerate(SR.COUNTS):
        assert np.array_equal(got_row[n].numpy(), counts_row[:, i]) and np.array_equal(got_lane[n].numpy(), counts_lane[:, i]), n
    assert np.array_equal(lane._score["last_id"].cpu().numpy(), last)
    sw_row, sw_lane = int(got_row["idsw"].sum()), int(got_lane["idsw"].sum())
    print("idsw on obj_id:", sw_row, "on lane_id:", sw_lane, "tp:", int(got_lane["tp"].sum()))
    assert int(got_lane["tp"].sum()) > 0 and sw_lane <= sw_row
    _check(lane, b, cfg=OPEN)
    row.close()
    lane.close()


def test_call_errors():
    F, P, obs, noise = _setup(1)
    st = _stream(F, P)
    with pytest.raises(ValueError, match="keeps no identities"):
        st.identities()
    st.close()
    with pytest.raises(ValueError, match=r"identity_tracks must be an integer in \[n_steps_per_image, 16\]"):
        _stream(F, P, identity=True, identity_tracks=N - 1)
    st = _stream(F, P, identity=True, identity_tracks=None)
    assert st.M == 2 * N and st._ident["trk_id"].shape == (B, 2 * N)
    st.close()
