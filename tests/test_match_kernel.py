"""-m gpu: keep + optimal per-frame matching on the device (sqair_set_lane_match; sq_assign_keep_optimal in k_lane_score_opt,
k_lane_identity_opt and k_lane_traj_score_opt), through the kernel-level entries on caller buffers.

Hand cases (tests/match_cases.py: hand): exact.  On the crowded cases of tests/match_cases.py -- 200 lanes, T = 8, (G, N) = (1, 1),
(2, 2), (4, 4), (3, 4) and (16, 14) on the wide library, iou_min 0.5 and 0.3 -- equally optimal assignments tie and the header states
no rule among them, so the device's matching is not compared with one reference matching.  It is JUDGED per scored (frame, lane)
(tests/match_ref.py: Judge): one-to-one, eligible pairs only, the keep honoured; its number of pairs equal to the float64 optimum's;
its sum of q, evaluated by the reference in float64 on the device's own pairs, at least the optimum's minus 2 min(rows, cols) (1 + e),
e the measured error of an fp32 restatement of sq_box_iou in units of 2^-20 (per pair q moves by rounding plus that error, on both
sides).  Then it is IMPOSED on the reference, which runs frame by frame on the device's pairs: events, memory and counters are
compared exactly, ``match_iou`` / ``link_iou`` within four times the restatement's measured error (the factor covers the device's
division, as in tests/test_score_kernel.py) and ``iou_sum`` within that times the lane's tp.  A lane is left out from its first
frame with a candidate IoU within 1e-5 of iou_min (at most 1 % of the lanes for the score: tests/test_match_ref.py holds the inputs
to that from the reference alone); no lane is left out for a tie.  The same for the identity's position link, (M, N) = (1, 1),
(4, 4), (8, 4) and (16, 14), and for the trajectory link.  Determinism: two passes of four frames equal one of eight bit for bit, a
captured graph equals eager calls and freezes the mode, mode 0 after mode 1 gives the bits of a handle that never set the mode, and
the setting outlives the registrations.  The IDF table fed the optimal ``truth_match`` gives the ``matched`` / ``frag`` of
tests/idf_ref.py on it.  With SQAIR_PARITY_DIR set the figures are added to match_parity.json there."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import identity_ref as I
from tests import idf_ref
from tests import match_cases as MC
from tests import match_ref as M
from tests import score_ref as R
from tests import traj_score_ref as TR
from tests.abi_host import open_handle
from tests.idf_cases import struct as idf_struct, to_device as idf_to_device
from tests.match_ref import record

pytestmark = pytest.mark.gpu

IDS = [MC.case_id(c) for c in MC.CASES]
INT_OUT = ("truth_match", "tp", "fn", "fp", "idsw")
IDENT_IN = ("box", "presence", "obj_id", "what", "best_row")
IDENT_IOU, IDENT_MAX_AGE = 0.3, 3
_handles = {}


def _handle(wide, N, fresh=False):
    key = (wide, N)
    if fresh or key not in _handles:
        opened = open_handle(_capi.WIDE_LIB_PATH if wide else None, MC.HW, k_particles=2, n_steps_per_image=N, n_what=MC.NW)
        if fresh:
            return opened
        _handles[key] = opened
    return _handles[key]


def _mode(lib, h, score=0, identity=0, traj=0):
    assert lib.sqair_set_lane_match(h, score, identity, traj) == 0, lib.sqair_last_error(h)


def _dev(x):
    return {k: torch.from_numpy(np.array(v)).cuda() for k, v in x.items()}


def _stream(stream=None):
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


# ---- the score ---------------------------------------------------------------------------------------------------------------------
def _score_state(B, G, last=None):
    last_id = torch.full((B, G), -1, dtype=torch.int32, device="cuda") if last is None else torch.from_numpy(np.array(last)).cuda()
    return dict(counts=torch.zeros((B, 9), dtype=torch.int64, device="cuda"), iou_sum=torch.zeros(B, dtype=torch.float64, device="cuda"),
                last_id=last_id)


def _score_out(T, B, G):
    shapes = _capi.score_shapes(T, B, G)
    return {n: torch.full(shapes[n], -7, dtype=torch.int32 if n in _capi.SCORE_INT_FIELDS else torch.float32, device="cuda")
            for n in _capi.SCORE_FIELDS}


def _score_launch(lib, h, x, state, out, G, iou_min, stream=None):
    """One launch of the score's kernel-level entry over the (contiguous, device) frames ``x``, continuing ``state`` in place."""
    T, B = x["map_count"].shape
    sc = _capi.SqairLaneScore(iou_min=iou_min, G=G, truth_box=x["truth_box"].data_ptr(), truth_present=x["truth_present"].data_ptr(),
                              truth_valid=x["truth_valid"].data_ptr(), **{n: t.data_ptr() for n, t in state.items()},
                              **{n: t.data_ptr() for n, t in out.items()})
    rc = lib.sqair_lane_score_test(h, x["box"].data_ptr(), x["presence"].data_ptr(), x["obj_id"].data_ptr(), x["map_count"].data_ptr(),
                                   T, B, C.byref(sc), _stream(stream))
    assert rc == 0, lib.sqair_last_error(h)


def _score_run(lib, h, d, state, G, iou_min, frames=slice(None)):
    x = {k: v[frames].contiguous() for k, v in d.items()}
    T, B = x["map_count"].shape
    out = _score_out(T, B, G)
    _score_launch(lib, h, x, state, out, G, iou_min)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in out.items()}


@functools.lru_cache(maxsize=None)
def _case(i):
    """The case's inputs on the host and on the device, e (units of 2^-20), the float tolerance and each lane's first fragile frame:
    made once, never written to."""
    c = MC.CASES[i]
    x = MC.make(c)
    err = R.iou32_error(x["truth_box"], x["box"])
    on = (x["truth_valid"] != 0) & (x["map_count"] != -1)
    first = M.fragile_from(R.iou_table(x["truth_box"], x["box"]), x["truth_present"], x["presence"], on, c.iou_min)
    return c, x, _dev(x), err * M.UNIT, 4.0 * err, first


@functools.lru_cache(maxsize=None)
def _optimal_score(i):
    """The device's optimal-mode run of the case (per-frame outputs, state), shared by the tests that read it."""
    c, x, d, _, _, _ = _case(i)
    lib, h = _handle(c.wide, c.N)
    _mode(lib, h, score=1)
    state = _score_state(MC.B, c.G)
    got = _score_run(lib, h, d, state, c.G, c.iou_min)
    _mode(lib, h)
    return got, {n: t.cpu().numpy() for n, t in state.items()}


def test_the_hand_cases_are_exact():
    x, last, expect, greedy = MC.hand()
    lib, h = _handle(False, MC.HAND_N)
    d = _dev(x)
    _mode(lib, h, score=1)
    got = _score_run(lib, h, d, _score_state(len(MC.HAND), MC.HAND_G, last), MC.HAND_G, MC.HAND_IOU)
    _mode(lib, h)
    grd = _score_run(lib, h, d, _score_state(len(MC.HAND), MC.HAND_G, last), MC.HAND_G, MC.HAND_IOU)
    lane = MC.HAND.index("cardinality")
    print("hand cases: tp optimal", got["tp"][0].tolist(), "greedy", grd["tp"][0].tolist())
    assert got["tp"][0, lane] == 2 and got["truth_match"][0, lane, :2].tolist() == [1, 0]          # the issue's frame: tp 2
    assert (grd["tp"][0, lane], grd["fn"][0, lane], grd["fp"][0, lane]) == (1, 1, 1)
    for n, want in expect.items():
        assert np.array_equal(got[n], want), (n, got[n], want)
    for n, want in greedy.items():
        assert np.array_equal(grd[n], want), (n, grd[n], want)
    s = MC.HAND.index("sum")
    assert abs(float(got["match_iou"][0, s].sum()) - 2 * 18 / 22) < 1e-6 and abs(float(grd["match_iou"][0, s].sum()) - (19 / 21 + 15 / 25)) < 1e-6


@pytest.mark.parametrize("i", range(len(MC.CASES)), ids=IDS)
def test_score_matching_is_optimal_and_the_events_follow_it(i):
    c, x, d, e, tol, first = _case(i)
    got, state = _optimal_score(i)
    frames = M.scored_frames(x)
    skip = [(t, b) for t, b in frames if t >= first[b]]
    judge = M.Judge([((t, b), got["truth_match"][t, b]) for t, b in frames], M.slack(e), skip)
    with M.replaced(R, "assign", judge.assign):
        ref = R.score(iou_min=c.iou_min, **x)
    whole = first == MC.T
    upto = np.arange(MC.T)[:, None] < first[None, :]
    left_out = int((~whole).sum())
    print(MC.case_id(c), "judged", judge.judged, "of", judge.asked, "left out", left_out, "worst deficit of the sum of q",
          judge.worst_deficit, "allowed", M.slack(e)(c.G, c.N), "e = {:.3f}".format(e))
    assert left_out <= MC.FRAGILE_CAP * MC.B and judge.asked == len(frames)
    bad = [k for k in judge.infeasible if k not in set(skip)]
    assert not bad, ("infeasible", bad[:4])
    assert not judge.cardinality, ("cardinality", judge.cardinality[:4])
    assert not judge.deficit, ("sum of q", judge.deficit[:4])
    for n in INT_OUT:
        assert np.array_equal(got[n][upto], getattr(ref, n)[upto]), (n, np.argwhere(got[n][upto] != getattr(ref, n)[upto])[:4])
    assert np.array_equal(state["counts"][whole], ref.counts[whole]), np.argwhere(state["counts"] != ref.counts)[:4]
    assert np.array_equal(state["last_id"][whole], ref.last_id[whole])
    err = float(np.abs(got["match_iou"].astype(np.float64) - ref.match_iou)[upto].max())
    err_sum = float((np.abs(state["iou_sum"] - ref.iou_sum) / np.maximum(ref.counts[:, 3], 1))[whole].max())
    tot = dict(zip(R.COUNTS, state["counts"].sum(0).tolist()))
    print(MC.case_id(c), "match_iou: largest error {:.3g}, iou_sum per tp {:.3g}; allowed {:.3g}".format(err, err_sum, tol), tot)
    record("kernel_score", MC.case_id(c), judged=judge.judged, left_out=left_out, worst_q_deficit=int(judge.worst_deficit),
           allowed_q_deficit=float(M.slack(e)(c.G, c.N)), match_iou=err, iou_sum_per_tp=err_sum, allowed=tol, **tot)
    assert tol < 1e-5 and err <= tol and (np.abs(state["iou_sum"] - ref.iou_sum) <= tol * ref.counts[:, 3])[whole].all()
    unscored = (x["truth_valid"] == 0) | (x["map_count"] == -1)
    assert all((got[n][unscored] == -1).all() for n in INT_OUT) and not got["match_iou"][unscored].any()
    assert state["counts"][MC.NAN_LANE, 1] == MC.T - MC.NAN_FROM and not state["counts"][MC.INVALID_LANE].any()


@pytest.mark.parametrize("i", [4, 9], ids=[IDS[4], IDS[9]])
def test_determinism_of_the_score(i):
    c, x, d, _, _, _ = _case(i)
    full, one = _optimal_score(i)
    lib, h = _handle(c.wide, c.N)
    bits = lambda a: a.view(np.int32) if a.dtype == np.float32 else a
    # two passes of four frames equal one of eight
    _mode(lib, h, score=1)
    two = _score_state(MC.B, c.G)
    a, b = _score_run(lib, h, d, two, c.G, c.iou_min, slice(0, 4)), _score_run(lib, h, d, two, c.G, c.iou_min, slice(4, 8))
    for n in _capi.SCORE_FIELDS:
        assert np.array_equal(bits(np.concatenate([a[n], b[n]])), bits(full[n])), n
    for n in one:
        assert np.array_equal(two[n].cpu().numpy().view(np.uint8), one[n].view(np.uint8)), n
    # a captured graph equals eager calls, and freezes the mode: it is replayed after the handle went back to greedy
    xs = {k: v.contiguous() for k, v in d.items()}
    gstate, gout = _score_state(MC.B, c.G), _score_out(MC.T, MC.B, c.G)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    assert lib.sqair_capture_begin(h, _stream(side)) == 0, lib.sqair_last_error(h)
    _score_launch(lib, h, xs, gstate, gout, c.G, c.iou_min, stream=side)
    assert lib.sqair_capture_end(h, _stream(side), 3) == 1, lib.sqair_last_error(h)      # one kernel node in either mode
    _mode(lib, h)
    assert lib.sqair_capture_launch(h, 3, _stream(side)) == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    for n in _capi.SCORE_FIELDS:
        assert np.array_equal(bits(gout[n].cpu().numpy()), bits(full[n])), n
    assert all(np.array_equal(gstate[n].cpu().numpy(), one[n]) for n in ("counts", "last_id"))
    assert np.array_equal(gstate["iou_sum"].cpu().numpy().view(np.int64), one["iou_sum"].view(np.int64))
    # mode 0 after mode 1: the bits of a handle that never set the mode
    back = _score_state(MC.B, c.G)
    after = _score_run(lib, h, d, back, c.G, c.iou_min)
    lib2, h2 = _handle(c.wide, c.N, fresh=True)
    never_state = _score_state(MC.B, c.G)
    never = _score_run(lib2, h2, d, never_state, c.G, c.iou_min)
    lib2.sqair_destroy(h2)
    for n in _capi.SCORE_FIELDS:
        assert np.array_equal(bits(after[n]), bits(never[n])), n
    assert all(torch.equal(back[n], never_state[n]) for n in back)
    assert not np.array_equal(after["truth_match"], full["truth_match"])                   # (and the modes do differ on these inputs)
    # the setting outlives the registrations going off: still optimal after sqair_set_score(NULL) and sqair_set_estimate(NULL)
    _mode(lib, h, score=1)
    assert lib.sqair_set_score(h, None, 0, 0) == 0 and lib.sqair_set_identity(h, None, 0, 0) == 0 and lib.sqair_set_estimate(h, None, 0, 0) == 0
    still = _score_run(lib, h, d, _score_state(MC.B, c.G), c.G, c.iou_min)
    _mode(lib, h)
    assert np.array_equal(still["truth_match"], full["truth_match"])


@pytest.mark.parametrize("i", [4, 9], ids=[IDS[4], IDS[9]])
def test_the_idf_table_follows_the_optimal_truth_match(i):
    c, x, d, _, _, first = _case(i)
    got, _ = _optimal_score(i)
    lib, h = _handle(c.wide, c.N)
    P = 32
    ids = R.words(x["obj_id"])
    table = idf_to_device(idf_ref.new_table(MC.B, c.G, P))
    tm = torch.from_numpy(got["truth_match"]).cuda()
    sc = _capi.SqairLaneScore(iou_min=c.iou_min, G=c.G, truth_box=d["truth_box"].data_ptr(), truth_present=d["truth_present"].data_ptr(),
                              truth_valid=d["truth_valid"].data_ptr(), truth_match=tm.data_ptr())
    _mode(lib, h, score=1)
    rc = lib.sqair_lane_idf_test(h, d["box"].data_ptr(), d["presence"].data_ptr(), d["obj_id"].data_ptr(), d["map_count"].data_ptr(), MC.T,
                                 MC.B, C.byref(sc), C.byref(idf_struct(table, P)), _stream())
    _mode(lib, h)
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    ref = idf_ref.accumulate(idf_ref.new_table(MC.B, c.G, P), x["box"], x["presence"], ids, x["map_count"], x["truth_box"],
                             x["truth_present"], x["truth_valid"], got["truth_match"], c.iou_min)
    whole = first == MC.T
    for n in ("matched", "frag", "trk_state", "row_frames", "frames"):
        assert np.array_equal(table[n].cpu().numpy()[whole], ref[n][whole]), n
    # (matched is the optimal mode's tp per truth: more than the greedy mode's on the same frames)
    grd = R.score(iou_min=c.iou_min, **x)
    assert int(ref["matched"].sum()) == int((got["truth_match"] >= 0).sum()) > int((grd.truth_match >= 0).sum())


# ---- the identity's position link --------------------------------------------------------------------------------------------------
IDENT_RUNS = [(0, 1, 0.0), (4, 4, 0.0), (4, 8, 0.0), (4, 8, 4.0), (8, 16, 0.0)]      # (case, M, reid_dist)
IDENT_IDS = ["{}_M{}{}".format(IDS[i], m, "_reid" if r else "") for i, m, r in IDENT_RUNS]


def _ident_memory(M_, appearance):
    mem = I.fresh_memory(MC.B, M_, MC.NW, appearance)
    return {k: torch.from_numpy(v).cuda() for k, v in mem.items() if v is not None}


def _ident_run(lib, h, d, mem, M_, reid, frames=slice(None)):
    x = {k: v[frames].contiguous() for k, v in d.items()}
    T, B, N = x["presence"].shape
    out = {n: torch.full((T, B, N), -7, dtype=torch.int32, device="cuda") for n in _capi.IDENT_FIELDS}
    idt = _capi.SqairLaneIdentity(iou_min=IDENT_IOU, reid_dist=reid, reid_what=float("inf"), M=M_, max_age=IDENT_MAX_AGE,
                                  **{n: t.data_ptr() for n, t in mem.items()}, **{n: t.data_ptr() for n, t in out.items()})
    rc = lib.sqair_lane_identity_test(h, *[x[k].data_ptr() for k in IDENT_IN], T, B, C.byref(idt), _stream())
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in out.items()}


@pytest.mark.parametrize("run", range(len(IDENT_RUNS)), ids=IDENT_IDS)
def test_identity_link_is_optimal_and_the_table_follows_it(run):
    i, M_, reid = IDENT_RUNS[run]
    c = MC.CASES[i]
    y = MC.identity_inputs(c)
    d = _dev(y)
    lib, h = _handle(c.wide, c.N)
    appearance = reid > 0.0
    _mode(lib, h, identity=1)
    mem = _ident_memory(M_, appearance)
    got = _ident_run(lib, h, d, mem, M_, reid)
    # two passes of four frames equal one of eight, bit for bit
    mem2 = _ident_memory(M_, appearance)
    a, b = _ident_run(lib, h, d, mem2, M_, reid, slice(0, 4)), _ident_run(lib, h, d, mem2, M_, reid, slice(4, 8))
    _mode(lib, h)
    assert all(np.array_equal(np.concatenate([a[n], b[n]]), got[n]) for n in got)
    assert all(np.array_equal(mem[n].cpu().numpy().view(np.uint8), mem2[n].cpu().numpy().view(np.uint8)) for n in mem)
    grd = _ident_run(lib, h, d, _ident_memory(M_, appearance), M_, reid)
    mem = {k: v.cpu().numpy() for k, v in mem.items()}
    # the reference, frame by frame on the device's own links (tests/match_ref.py: IdentityFollower)
    e_units = R.iou32_error(y["box"][:-1], y["box"][1:]) * M.UNIT         # (a track's box is a slot's box of an earlier frame)
    tol = I.measured_tol(y["box"], y["best_row"], y["what"], appearance) if reid > 0.0 else None
    kw = dict(iou_min=IDENT_IOU, reid_dist=reid, reid_what=float("inf"), M=M_, max_age=IDENT_MAX_AGE, appearance=appearance)
    follower = M.IdentityFollower(MC.B, c.N, MC.NW, kw, e_units, tol)
    out = follower.feed(y, got["how"], got["lane_id"])
    ref_mem, failures, asked, judged, worst = follower.mem, follower.failures, follower.asked, follower.judged, follower.worst
    whole, upto = follower.whole(), follower.upto()
    linked = lambda how: int(((how == I.KEPT) | (how == I.BRIDGED)).sum())
    print(IDENT_IDS[run], "judged", judged, "of", asked, "left out", int((~whole).sum()), "worst deficit", worst, "allowed",
          M.slack(e_units)(M_, c.N), "position links optimal", linked(got["how"]), "greedy", linked(grd["how"]))
    record("kernel_identity", IDENT_IDS[run], judged=judged, left_out=int((~whole).sum()), worst_q_deficit=int(worst),
           allowed_q_deficit=float(M.slack(e_units)(M_, c.N)), links_optimal=linked(got["how"]), links_greedy=linked(grd["how"]))
    assert not failures, failures[:4]
    assert (~whole).sum() <= 0.05 * MC.B          # (the link has its own tables, the track boxes: not the score's cap, but few)
    for n in out:
        assert np.array_equal(got[n][upto], out[n][upto]), (n, np.argwhere(got[n] != out[n])[:4])
    for n in ("trk_id", "trk_word", "trk_age", "trk_len", "next_id", "counts"):
        assert np.array_equal(mem[n][whole], ref_mem[n][whole]), n
    live = ref_mem["trk_id"] >= 0
    assert np.array_equal(mem["trk_box"][whole].view(np.int32)[live[whole]], ref_mem["trk_box"][whole].view(np.int32)[live[whole]])
    if c.N >= 2:
        assert linked(got["how"]) > linked(grd["how"])


# ---- the trajectory link -----------------------------------------------------------------------------------------------------------
def _traj_launch(lib, h, c, dev, state, out, iou_min):
    tab = _capi.SqairLaneTraj(**{n: dev[n].data_ptr() for n in _capi.TRAJ_TABLE_FIELDS if n in dev})
    tru = _capi.SqairTrajTruth(G=c.G, **{n: dev[n].data_ptr() for n in _capi.TRAJ_TRUTH_FIELDS if n in dev})
    sco = _capi.SqairTrajScore(iou_min=iou_min, **{n: t.data_ptr() for n, t in state.items()}, **{n: t.data_ptr() for n, t in out.items()})
    rc = lib.sqair_lane_traj_score(h, C.byref(tab), C.byref(tru), C.byref(sco), MC.TRAJ_F, MC.B, _stream())
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()


def _traj_buffers(c):
    z = lambda shp, dt: torch.zeros(shp, dtype=dt, device="cuda")
    F = MC.TRAJ_F
    state = dict(counts=z((F, MC.B, len(TR.COUNTS)), torch.int64), sums=z((F, MC.B, len(TR.SUMS)), torch.float64),
                 lane_counts=z((MC.B, len(TR.LANE_COUNTS)), torch.int64))
    shapes = _capi.traj_shapes(F, MC.B, c.G)
    out = {n: torch.full(shapes[n], -7, dtype=torch.int32 if n in _capi.TRAJ_INT_FIELDS else torch.float32, device="cuda")
           for n in _capi.TRAJ_FIELDS}
    return state, out


@pytest.mark.parametrize("i", [2, 4, 7, 9], ids=[IDS[i] for i in (2, 4, 7, 9)])
@pytest.mark.parametrize("keep", [False, True], ids=["", "keep_id"])
def test_trajectory_link_is_optimal_and_the_counts_follow_it(i, keep):
    c = MC.CASES[i]
    tab, tr, keep_id = MC.traj_inputs(c)
    keep_id = keep_id if keep else None
    dev = _dev(dict(tab, **tr))
    if keep:
        dev["keep_id"] = torch.from_numpy(np.array(keep_id)).cuda()
    lib, h = _handle(c.wide, c.N)
    _mode(lib, h, traj=1)
    state, out = _traj_buffers(c)
    _traj_launch(lib, h, c, dev, state, out, c.iou_min)
    state2, out2 = _traj_buffers(c)
    _traj_launch(lib, h, c, dev, state2, out2, c.iou_min)                       # (the same bits on a second call)
    _mode(lib, h)
    gstate, gout = _traj_buffers(c)
    _traj_launch(lib, h, c, dev, gstate, gout, c.iou_min)
    got = {n: t.cpu().numpy() for n, t in out.items()}
    assert all(np.array_equal(got[n].view(np.int32), out2[n].cpu().numpy().view(np.int32)) for n in got)
    assert all(torch.equal(state[n], state2[n]) for n in ("counts", "lane_counts"))
    on = TR.lane_on(tab, tr)
    iou = TR.anchor_iou(tab, tr)
    e = float(np.abs(TR.anchor_iou(tab, tr, np.float32).astype(np.float64) - iou).max())
    near = M.fragile_from(iou[None], tr["anchor_present"][None], tab["presence"][None], on[None], c.iou_min) == 0
    lanes = np.nonzero(on)[0]
    judge = M.Judge([(int(b), got["link"][b]) for b in lanes], M.slack(e * M.UNIT), [int(b) for b in lanes if near[b]])
    with M.replaced(TR, "assign", judge.assign):
        ref = TR.score(tab, tr, c.iou_min, keep_id)
    whole = ~near
    print(MC.case_id(c), "keep_id" if keep else "", "judged", judge.judged, "of", judge.asked, "left out", int(near.sum()), "worst deficit",
          judge.worst_deficit, "linked optimal", int(state["lane_counts"][:, 3].sum()), "greedy", int(gstate["lane_counts"][:, 3].sum()))
    record("kernel_traj_link", MC.case_id(c) + ("_keep_id" if keep else ""), judged=judge.judged, left_out=int(near.sum()),
           worst_q_deficit=int(judge.worst_deficit), linked_optimal=int(state["lane_counts"][:, 3].sum()),
           linked_greedy=int(gstate["lane_counts"][:, 3].sum()))
    assert [k for k in judge.infeasible if not near[k]] == [] and not judge.cardinality and not judge.deficit, (
        judge.infeasible[:4], judge.cardinality[:4], judge.deficit[:4])
    assert np.array_equal(got["link"][whole], ref.link[whole]) and np.array_equal(got["state"][:, whole], ref.state[:, whole])
    assert np.array_equal(state["lane_counts"].cpu().numpy()[whole], ref.lane_counts[whole])
    counts = state["counts"].cpu().numpy()
    for k in (0, 1, 3, 4, 5, 6):                  # (hits hangs on pair_iou >= iou_min, another compare: tests/test_traj_score_kernel.py's)
        assert np.array_equal(counts[:, whole, k], ref.counts[:, whole, k]), TR.COUNTS[k]
    assert float(np.abs(got["link_iou"].astype(np.float64) - ref.link_iou)[whole].max()) <= 4.0 * e < 1e-5
    assert state["lane_counts"][:, 3].sum() > gstate["lane_counts"][:, 3].sum()
