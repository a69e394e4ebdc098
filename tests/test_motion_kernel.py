"""-m gpu: the identity kernel's motion instantiation (k_lane_identity_motion / _motion_opt, through sqair_lane_identity_motion_test)
against the float64 reference of tests/motion_ref.py, on caller buffers, for the cases of tests/motion_cases.py: 200 lanes, T = 12,
(M, N, n_what) = (8, 4, 50), (4, 4, 50) -- every birth evicts --, (1, 1, 1) and (16, 14, 128) on the wide library, one case without
trk_what, one with the position link keep + optimal.

The integer outputs (``lane_id``, ``how``, ``track_len``), the integer memory and ``counts`` are compared exactly, ``trk_box`` and
``trk_what`` as bits.  ``velocity``, ``nis`` and ``trk_kf`` (the live entries of the lanes compared to the end) are compared within a
bar that is MEASURED: per case four times the largest error of the fp32 restatement of the filter against float64 over the compared
lanes (tests/motion_ref.py) -- the margin of the fragility band, which covers the freedom the compiler has over the restatement's
order.  A lane is left out from its first fragile frame on, at most 2 % of the lanes; tests/test_motion_ref.py holds the same inputs
to that cap from the reference alone.  Also here: two passes of six frames leave the bits of one pass of twelve, a captured graph
replayed twice leaves the bits of eager calls, ``nis`` is optional, a NULL motion gives the bits of sqair_lane_identity_test, and the
two hand-made scenarios (a fast mover, a moving drop-out) keep one id where the kernel without the filter gives a fresh one.  With
SQAIR_PARITY_DIR set the measured figures are written to motion_parity.json there (the copy under profiles/ is such a file)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import identity_ref as IR
from tests import motion_cases as MC
from tests import motion_ref as MR
from tests.abi_host import open_handle
from tests.kernel_unit import merge_parity

pytestmark = pytest.mark.gpu

INPUTS = ("box", "presence", "obj_id", "what", "best_row")
INT_MEM = ("trk_word", "trk_age", "trk_len")
NOTE = ("per case of tests/test_motion_kernel.py: the fragility band (four times the measured error of the fp32 restatement of IoU, "
        "d2 and dw against float64), the lanes left out as fragile, the bars of velocity, nis and trk_kf (four times the restatement's "
        "error over the lanes compared), the kernel's own error against float64 and the events counted over the lanes compared; the "
        "integer outputs, the memory and counts are compared exactly")


def _record(case, **figures):
    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data["cases"][case] = figures
    merge_parity("motion_parity.json", lambda: {"note": NOTE, "cases": {}}, update)


_handles = {}


def _handle(wide, N, nw, optimal=False):
    key = (wide, N, nw, optimal)
    if key not in _handles:
        lib, h = open_handle(_capi.WIDE_LIB_PATH if wide else None, MC.HW, k_particles=2, n_steps_per_image=N, n_what=nw)
        assert lib.sqair_set_lane_match(h, 0, int(optimal), 0) == 0
        _handles[key] = lib, h
    return _handles[key]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """The case's inputs on the host and on the device, the reference and the lanes compared: made once, never written to."""
    x, ref, tol, first = MC.reference(i)
    return x, {k: torch.from_numpy(v).cuda() for k, v in x.items()}, ref, tol, first


def _memory(B, M, nw, appearance):
    mem = IR.fresh_memory(B, M, nw, appearance)
    mem = {k: torch.from_numpy(v).cuda() for k, v in mem.items() if v is not None}
    mem["trk_kf"] = torch.zeros((B, M, 2, 5), dtype=torch.float32, device="cuda")
    return mem


def _launch(lib, h, x, mem, M, reid_dist, max_age, motion=True, nis=True, fields=_capi.IDENT_FIELDS, stream=None, out=None):
    """One launch over the frames ``x`` (device tensors), continuing ``mem`` in place; returns the per-frame outputs (device)."""
    T, B, N = x["presence"].shape
    o = out if out is not None else _outputs(T, B, N, nis, fields)
    idt = _capi.SqairLaneIdentity(iou_min=MC.IOU_MIN, reid_dist=reid_dist, reid_what=float("inf"), M=M, max_age=max_age,
                                  **{n: t.data_ptr() for n, t in mem.items() if n != "trk_kf"},
                                  **{n: o[n].data_ptr() for n in fields})
    mo = _capi.SqairLaneMotion(q=MC.Q, r=MC.R_MEAS, v0_var=MC.V0_VAR, gate=MC.GATE, trk_kf=mem["trk_kf"].data_ptr(),
                               velocity=o["velocity"].data_ptr(), nis=o["nis"].data_ptr() if nis else None)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream) if stream is None else stream
    rc = lib.sqair_lane_identity_motion_test(h, *[x[k].data_ptr() for k in INPUTS], T, B, C.byref(idt), C.byref(mo) if motion else None, s)
    assert rc == 0, lib.sqair_last_error(h)
    return o


def _outputs(T, B, N, nis=True, fields=_capi.IDENT_FIELDS):
    o = {n: torch.full((T, B, N), -7, dtype=torch.int32, device="cuda") for n in fields}
    o["velocity"] = torch.full((T, B, N, 2), -7.0, device="cuda")
    if nis:
        o["nis"] = torch.full((T, B, N), -7.0, device="cuda")
    return o


def _run(c, d, mem, frames=slice(None), **kw):
    lib, h = _handle(c.wide, c.N, c.nw, c.optimal)
    o = _launch(lib, h, {k: v[frames].contiguous() for k, v in d.items()}, mem, c.M, MC.REID_DIST, MC.MAX_AGE, **kw)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return all(torch.equal(a[n].view(torch.int32) if a[n].dtype == torch.float32 else a[n],
                           b[n].view(torch.int32) if b[n].dtype == torch.float32 else b[n]) for n in a)


@pytest.mark.parametrize("i", range(len(MC.CASES)), ids=[MC.case_id(c) for c in MC.CASES])
def test_motion_kernel_against_fp64(i):
    c = MC.CASES[i]
    x, d, ref, tol, first = _inputs(i)
    mem = _memory(MC.B, c.M, c.nw, c.appearance)
    got = _run(c, d, mem)
    mem = {k: v.cpu().numpy() for k, v in mem.items()}
    whole = first == MC.T                                          # lanes compared to the end
    upto = np.arange(MC.T)[:, None] < first[None, :]               # [T, B]: frames before a lane's first fragile one
    left_out = int((~whole).sum())
    bars = MR.bars(ref.err, whole)
    print(MC.case_id(c), "lanes left out as fragile:", left_out, "of", MC.B, "band", tol, "bars", bars)
    assert left_out <= MC.FRAGILE_CAP * MC.B
    for n in _capi.IDENT_FIELDS:
        want = getattr(ref, n)
        assert got[n].dtype == np.int32 and np.array_equal(got[n][upto], want[upto]), (n, np.argwhere((got[n] != want) & upto[..., None])[:4])
    rm = ref.mem
    assert np.array_equal(mem["trk_id"][whole], rm["trk_id"][whole]), np.argwhere(mem["trk_id"] != rm["trk_id"])[:4]
    assert np.array_equal(mem["next_id"][whole], rm["next_id"][whole])
    assert np.array_equal(mem["counts"][whole], rm["counts"][whole]), np.argwhere(mem["counts"] != rm["counts"])[:4]
    for n in INT_MEM + ("trk_box",) + (("trk_what",) if c.appearance else ()):      # (free entries too: what they last held)
        assert np.array_equal(_bits(mem[n])[whole], _bits(rm[n])[whole]), n
    # the filter: velocity and nis of the frames compared, the state of the live entries of the lanes compared to the end
    live = whole[:, None] & (rm["trk_id"] >= 0)
    errs = dict(velocity=float(np.abs(got["velocity"] - ref.velocity)[upto].max()), nis=float(np.abs(got["nis"] - ref.nis)[upto].max()),
                kf=float(np.abs(mem["trk_kf"] - rm["trk_kf"])[live].max()))
    print(MC.case_id(c), "the kernel's error against float64", errs)
    assert got["velocity"].dtype == got["nis"].dtype == np.float32 and np.isfinite(got["velocity"]).all() and np.isfinite(got["nis"]).all()
    for n in errs:
        assert 0.0 < bars[n] and errs[n] <= bars[n], (n, errs[n], bars[n])
    # the non-finite lane: -1 and 0 from NAN_FROM on, nothing else moved; the empty lane: frames and nothing else
    assert all((got[n][MC.NAN_FROM:, MC.NAN_LANE] == -1).all() for n in _capi.IDENT_FIELDS)
    assert (got["velocity"][MC.NAN_FROM:, MC.NAN_LANE] == 0).all() and (got["nis"][MC.NAN_FROM:, MC.NAN_LANE] == 0).all()
    assert mem["counts"][MC.NAN_LANE, 0] == MC.NAN_FROM and mem["counts"][MC.NAN_LANE, 1] == MC.T - MC.NAN_FROM
    assert mem["counts"][MC.EMPTY_LANE].tolist() == [MC.T] + [0] * 7 and (mem["trk_id"][MC.EMPTY_LANE] == -1).all()
    assert (mem["trk_kf"][MC.EMPTY_LANE] == 0).all()
    absent = (x["presence"] == 0) & (x["best_row"] != -1)[..., None]
    assert all((got[n][absent] == -1).all() for n in _capi.IDENT_FIELDS) and (got["velocity"][absent] == 0).all() and (got["nis"][absent] == 0).all()
    born = (got["how"] == MR.BORN) & upto[..., None]
    assert (got["velocity"][born] == 0).all() and (got["nis"][born] == 0).all()
    tot = dict(zip(MR.COUNTS, mem["counts"][whole].sum(0).tolist()))
    print(MC.case_id(c), tot)
    _record(MC.case_id(c), band=dict(tol._asdict()), bars=bars, kernel_error=errs, lanes=MC.B, left_out=left_out, **tot)
    assert all(tot[n] > 0 for n in ("kept", "bridged", "reidentified", "born", "ended")), tot
    assert tot["objects"] == tot["kept"] + tot["bridged"] + tot["reidentified"] + tot["born"]


@pytest.mark.parametrize("i", [0, 3, 4], ids=[MC.case_id(MC.CASES[i]) for i in (0, 3, 4)])
def test_two_passes_equal_one_and_nis_is_optional(i):
    c = MC.CASES[i]
    d = _inputs(i)[1]
    one = _memory(MC.B, c.M, c.nw, c.appearance)
    full = _run(c, d, one)
    two = _memory(MC.B, c.M, c.nw, c.appearance)
    a, b = _run(c, d, two, slice(0, 6)), _run(c, d, two, slice(6, 12))
    for n in full:
        assert np.array_equal(_bits(np.concatenate([a[n], b[n]])), _bits(full[n])), n
    assert _same(one, two)
    st = _memory(MC.B, c.M, c.nw, c.appearance)
    part = _run(c, d, st, nis=False, fields=("lane_id",))          # nis, how and track_len are optional
    assert set(part) == {"lane_id", "velocity"} and all(np.array_equal(_bits(part[n]), _bits(full[n])) for n in part)
    assert _same(one, st)


@pytest.mark.parametrize("i", [0, 5], ids=[MC.case_id(MC.CASES[i]) for i in (0, 5)])
def test_a_null_motion_gives_the_bits_of_the_identity_entry(i):
    c = MC.CASES[i]
    d = _inputs(i)[1]
    lib, h = _handle(c.wide, c.N, c.nw, c.optimal)
    a, b = _memory(MC.B, c.M, c.nw, c.appearance), _memory(MC.B, c.M, c.nw, c.appearance)
    got = _run(c, d, a, motion=False)
    o = _outputs(MC.T, MC.B, c.N)
    idt = _capi.SqairLaneIdentity(iou_min=MC.IOU_MIN, reid_dist=MC.REID_DIST, reid_what=float("inf"), M=c.M, max_age=MC.MAX_AGE,
                                  **{n: t.data_ptr() for n, t in b.items() if n != "trk_kf"}, **{n: o[n].data_ptr() for n in _capi.IDENT_FIELDS})
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.sqair_lane_identity_test(h, *[d[k].data_ptr() for k in INPUTS], MC.T, MC.B, C.byref(idt), s) == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    assert all(np.array_equal(got[n], o[n].cpu().numpy()) for n in _capi.IDENT_FIELDS) and _same(a, b)
    assert (got["velocity"] == -7).all() and (got["nis"] == -7).all() and (a["trk_kf"] == 0).all()      # nothing of the motion is touched
    # and the motion changes the answer: the same inputs, other ids
    assert not np.array_equal(_run(c, d, _memory(MC.B, c.M, c.nw, c.appearance))["lane_id"], got["lane_id"])


def test_a_replayed_graph_leaves_the_bits_of_eager_calls():
    """One launch of six frames captured once (sqair_capture_begin / _end) and replayed twice, on the first and then on the second half
    of the case, against two eager launches: the table and the filter's state are read, updated and written in place by the lane's
    one workgroup, so a replay continues them as an eager call does."""
    c = MC.CASES[0]
    d = _inputs(0)[1]
    lib, h = _handle(c.wide, c.N, c.nw, c.optimal)
    eager = _memory(MC.B, c.M, c.nw, c.appearance)
    want = [_run(c, d, eager, slice(0, 6)), _run(c, d, eager, slice(6, 12))]
    mem = _memory(MC.B, c.M, c.nw, c.appearance)
    halves = [{k: v[f].contiguous() for k, v in d.items()} for f in (slice(0, 6), slice(6, 12))]
    x = {k: v.clone() for k, v in halves[0].items()}           # the graph's input buffers
    o = _outputs(6, MC.B, c.N)
    side = torch.cuda.Stream()
    before = {k: v.clone() for k, v in mem.items()}
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    _launch(lib, h, x, mem, c.M, MC.REID_DIST, MC.MAX_AGE, stream=ss, out=o)
    assert lib.sqair_capture_end(h, ss, 3) == 1, lib.sqair_last_error(h)      # one launch: one kernel node
    torch.cuda.synchronize()
    assert _same(before, mem)                                  # (a capture launches nothing: the memory is as it was)
    for half, w in zip(halves, want):
        for k in x:
            x[k].copy_(half[k])
        torch.cuda.synchronize()
        assert lib.sqair_capture_launch(h, 3, ss) == 0, lib.sqair_last_error(h)
        torch.cuda.synchronize()
        for n in w:
            assert np.array_equal(_bits(o[n].cpu().numpy()), _bits(w[n])), n
    assert _same(eager, mem)


# ---- the two scenarios: one 10 x 10 object per lane, through the kernel entry ------------------------------------------------------
def _scenario(x, reid_dist, max_age, motion=True, frames=None):
    """The kernel on a scenario's inputs (M = N = 1, no trk_what): (the outputs, the memory), host arrays."""
    lib, h = _handle(False, 1, 1)
    x = {k: torch.from_numpy(v if frames is None else v[:frames]).cuda() for k, v in x.items()}
    mem = _memory(1, 1, 1, False)
    o = _launch(lib, h, x, mem, 1, reid_dist, max_age, motion=motion)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}, {n: t.cpu().numpy() for n, t in mem.items()}


def _velocity_bar():
    """The measured bar of this file's (1, 1, 1) case: the scenarios run on its handle and its shape."""
    _, _, ref, _, first = _inputs(2)
    return MR.bars(ref.err, first == MC.T)["velocity"]


@pytest.mark.parametrize("step", [(8.0, 0.0), (6.0, 6.0)], ids=["along_y", "diagonal"])
def test_the_fast_mover_keeps_one_id(step):
    x = MC.fast_mover(step)
    plain, _ = _scenario(x, 4.0, 10, motion=False)
    assert plain["lane_id"].ravel().tolist() == [0, 1, 2, 3, 4, 5] and (plain["how"] == MR.BORN).all()      # a fresh id every frame
    got, mem = _scenario(x, 4.0, 10)
    ref = MR.scenario_run(x, 4.0, 10, MC.SCALARS)
    assert got["lane_id"].ravel().tolist() == [0] * 6 and got["how"].ravel().tolist() == [0, 3, 1, 1, 1, 1]
    assert got["track_len"].ravel().tolist() == [1, 2, 3, 4, 5, 6] and mem["next_id"].tolist() == [1]
    bar = _velocity_bar()
    print(step, "velocity", got["velocity"][:, 0, 0].tolist(), "nis", got["nis"].ravel().tolist(), "bar", bar)
    assert np.abs(got["velocity"] - ref.velocity).max() <= bar
    assert abs(got["nis"][1, 0, 0] - ref.nis[1, 0, 0]) < 1e-4 and got["nis"][1, 0, 0] <= 9.0
    if step == (8.0, 0.0):
        assert np.allclose(got["velocity"][1:4, 0, 0, 0], [7.14, 7.80, 7.96], atol=0.005) and abs(got["nis"][1, 0, 0] - 3.54) < 0.005


@pytest.mark.parametrize("sigma", [0.0, 0.5], ids=["clean", "noisy"])
def test_the_moving_drop_out_keeps_its_id(sigma):
    x, true = MC.moving_dropout(sigma)
    plain, _ = _scenario(x, 2.0, 10, motion=False)
    assert plain["lane_id"].ravel()[[4, 9, 10]].tolist() == [0, 1, 1] and plain["how"][9, 0, 0] == MR.BORN      # born again at frame 9
    got, _ = _scenario(x, 2.0, 10)
    ref = MR.scenario_run(x, 2.0, 10, MC.SCALARS)
    assert got["lane_id"].ravel().tolist() == [0] * 5 + [-1] * 4 + [0, 0]
    assert got["how"].ravel().tolist() == [0, 1, 1, 1, 1, -1, -1, -1, -1, 1, 1] == ref.how.ravel().tolist()
    assert np.abs(got["velocity"] - ref.velocity).max() <= _velocity_bar()
    _, at8 = _scenario(x, 2.0, 10, frames=9)                      # the unseen track, coasted to frame 8
    assert at8["trk_age"].tolist() == [[4]] and at8["trk_id"].tolist() == [[0]]
    if sigma == 0.0:
        pred_box = np.concatenate([at8["trk_kf"][0, 0, :, 0] - 0.5 * at8["trk_box"][0, 0, 2:], at8["trk_box"][0, 0, 2:]])
        assert np.abs(pred_box - np.concatenate([true[8] - 5.0, [10.0, 10.0]])).max() < 0.1
        assert abs(got["velocity"][3, 0, 0, 0] - 2.98) < 0.005 and abs(got["velocity"][4, 0, 0, 0] - 3.0) < 0.005
