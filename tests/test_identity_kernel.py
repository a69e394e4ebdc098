"""-m gpu: the identity kernel (k_lane_identity, through sqair_lane_identity_test) against the float64 reference of
tests/identity_ref.py, on caller buffers, for the cases of tests/identity_cases.py: 200 lanes, T = 8, (M, N, n_what) = (8, 4, 50),
(4, 4, 50) -- a full table in which every birth evicts --, (1, 1, 1) and (16, 14, 128) on the wide library -- 224 threads fill the
tables there --, one case without trk_what, one with a finite reid_what, one with re-identification off.

Every output (``lane_id``, ``how``, ``track_len``), the whole memory and ``counts`` are compared exactly: they are integers, and
``trk_box`` / ``trk_what`` are word copies, compared as bits.  A lane is left out from its first fragile frame on
(tests/identity_ref.py: a decisive compare inside four times the measured error of the fp32 restatement of IoU, dc2 and dw), at most
2 % of the lanes -- tests/test_identity_ref.py holds the same inputs to that cap from the reference alone.  The fields of a FREE entry
other than trk_id are whatever they last held (the header says so): freeing is one store in the reference too, so they are compared
with the rest.  Also here: two passes of four frames give the
bits of one pass of eight (the memory and the counters are handed on in place), a captured graph replayed gives the bits of eager
calls, ``how`` and ``track_len`` are optional, and every case exercises all five events where it can.  With SQAIR_PARITY_DIR set the
measured figures are written to identity_parity.json there (the copy under profiles/ is such a file); without it nothing is written."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import identity_cases as IC
from tests import identity_ref as IR
from tests.abi_host import open_handle
from tests.kernel_unit import merge_parity

pytestmark = pytest.mark.gpu

INPUTS = ("box", "presence", "obj_id", "what", "best_row")
INT_MEM = ("trk_word", "trk_age", "trk_len")
NOTE = ("per case of tests/test_identity_kernel.py: the measured error of the fp32 restatement of IoU, dc2 and dw against "
        "float64 times four (the fragility band), the lanes left out as fragile and the events counted over the lanes "
        "compared; outputs, memory and counts are compared exactly")


def _record(case, **figures):
    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data["cases"][case] = figures
    merge_parity("identity_parity.json", lambda: {"note": NOTE, "cases": {}}, update)


_handles = {}


def _handle(c):
    key = (c.wide, c.N, c.nw)
    if key not in _handles:
        _handles[key] = open_handle(_capi.WIDE_LIB_PATH if c.wide else None, IC.HW, k_particles=2, n_steps_per_image=c.N, n_what=c.nw)
    return _handles[key]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """The case's inputs on the host and on the device, the reference and the lanes compared: made once, never written to."""
    c = IC.CASES[i]
    x = IC.make(c)
    d = {k: torch.from_numpy(v).cuda() for k, v in x.items()}
    tol = IR.measured_tol(x["box"], x["best_row"], x["what"], c.appearance)
    ref = IR.identity(iou_min=IC.IOU_MIN, reid_dist=c.reid_dist, reid_what=c.reid_what, M=c.M, max_age=IC.MAX_AGE,
                      appearance=c.appearance, tol=tol, **x)
    return x, d, ref, tol


def _memory(c):
    mem = IR.fresh_memory(IC.B, c.M, c.nw, c.appearance)
    return {k: torch.from_numpy(v).cuda() for k, v in mem.items() if v is not None}


def _struct(c, mem, out):
    return _capi.SqairLaneIdentity(iou_min=IC.IOU_MIN, reid_dist=c.reid_dist, reid_what=c.reid_what, M=c.M, max_age=IC.MAX_AGE,
                                   **{n: t.data_ptr() for n, t in mem.items()}, **{n: t.data_ptr() for n, t in out.items()})


def _outputs(c, T, fields):
    return {n: torch.full((T, IC.B, c.N), -7, dtype=torch.int32, device="cuda") for n in fields}


def _run(c, d, mem, frames=slice(None), fields=_capi.IDENT_FIELDS):
    """One launch over ``frames`` of the case, continuing ``mem`` in place; returns the per-frame outputs asked for."""
    lib, h = _handle(c)
    x = {k: v[frames].contiguous() for k, v in d.items()}
    T = x["best_row"].shape[0]
    o = _outputs(c, T, fields)
    idt = _struct(c, mem, o)
    s = torch.cuda.current_stream()
    rc = lib.sqair_lane_identity_test(h, *[x[k].data_ptr() for k in INPUTS], T, IC.B, C.byref(idt), C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in o.items()}


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.mark.parametrize("i", range(len(IC.CASES)), ids=[IC.case_id(c) for c in IC.CASES])
def test_identity_kernel_against_fp64(i):
    c = IC.CASES[i]
    x, d, ref, tol = _inputs(i)
    mem = _memory(c)
    got = _run(c, d, mem)
    mem = {k: v.cpu().numpy() for k, v in mem.items()}
    first = ref.fragile_from
    whole = first == IC.T                                          # lanes compared to the end
    upto = np.arange(IC.T)[:, None] < first[None, :]               # [T, B]: frames before a lane's first fragile one
    left_out = int((~whole).sum())
    print(IC.case_id(c), "lanes left out as fragile:", left_out, "of", IC.B, "band", tol)
    assert left_out <= IC.FRAGILE_CAP * IC.B
    for n in _capi.IDENT_FIELDS:
        want = getattr(ref, n)
        assert got[n].dtype == np.int32 and np.array_equal(got[n][upto], want[upto]), (n, np.argwhere((got[n] != want) & upto[..., None])[:4])
    rm = ref.mem
    assert np.array_equal(mem["trk_id"][whole], rm["trk_id"][whole]), np.argwhere(mem["trk_id"] != rm["trk_id"])[:4]
    assert np.array_equal(mem["next_id"][whole], rm["next_id"][whole])
    assert np.array_equal(mem["counts"][whole], rm["counts"][whole]), np.argwhere(mem["counts"] != rm["counts"])[:4]
    for n in INT_MEM + ("trk_box",) + (("trk_what",) if c.appearance else ()):      # (free entries too: what they last held)
        assert np.array_equal(_bits(mem[n])[whole], _bits(rm[n])[whole]), n
    # the non-finite lane: -1 from NAN_FROM on, nothing else moved; the empty lane: frames and nothing else
    assert all((got[n][IC.NAN_FROM:, IC.NAN_LANE] == -1).all() for n in _capi.IDENT_FIELDS)
    assert mem["counts"][IC.NAN_LANE, 0] == IC.NAN_FROM and mem["counts"][IC.NAN_LANE, 1] == IC.T - IC.NAN_FROM
    assert mem["counts"][IC.EMPTY_LANE].tolist() == [IC.T] + [0] * 7 and (mem["trk_id"][IC.EMPTY_LANE] == -1).all()
    absent = (x["presence"] == 0) & (x["best_row"] != -1)[..., None]
    assert all((got[n][absent] == -1).all() for n in _capi.IDENT_FIELDS)
    tot = dict(zip(IR.COUNTS, mem["counts"][whole].sum(0).tolist()))
    print(IC.case_id(c), tot)
    _record(IC.case_id(c), band=dict(tol._asdict()), lanes=IC.B, left_out=left_out, **tot)
    # all five events are exercised (re-identification where it is on)
    need = ("kept", "bridged", "born", "ended") + (("reidentified",) if c.reid_dist > 0 else ())
    assert all(tot[n] > 0 for n in need), tot
    assert c.reid_dist > 0 or tot["reidentified"] == 0
    assert tot["objects"] == tot["kept"] + tot["bridged"] + tot["reidentified"] + tot["born"]


@pytest.mark.parametrize("i", [0, 4, 5], ids=[IC.case_id(IC.CASES[i]) for i in (0, 4, 5)])
def test_two_passes_equal_one_and_the_outputs_are_optional(i):
    c = IC.CASES[i]
    _, d, _, _ = _inputs(i)
    one = _memory(c)
    full = _run(c, d, one)
    two = _memory(c)
    a, b = _run(c, d, two, slice(0, 4)), _run(c, d, two, slice(4, 8))
    for n in _capi.IDENT_FIELDS:
        assert np.array_equal(np.concatenate([a[n], b[n]]), full[n]), n
    for n in one:
        assert torch.equal(one[n].view(torch.int32) if one[n].dtype == torch.float32 else one[n],
                           two[n].view(torch.int32) if two[n].dtype == torch.float32 else two[n]), n
    for fields in (("lane_id",), ("lane_id", "how"), ("lane_id", "track_len")):      # how and track_len are optional
        st = _memory(c)
        part = _run(c, d, st, fields=fields)
        assert all(np.array_equal(part[n], full[n]) for n in fields)
        assert all(torch.equal(one[n].view(torch.int32) if one[n].dtype == torch.float32 else one[n],
                               st[n].view(torch.int32) if st[n].dtype == torch.float32 else st[n]) for n in one), fields


def test_a_replayed_graph_leaves_the_bits_of_eager_calls():
    """One launch of four frames captured once (sqair_capture_begin / _end) and replayed twice, on the first and then on the second half
    of the case, against two eager launches: the memory is read, updated and written
    in place by the lane's one workgroup, so a replay continues it as an eager call does."""
    c = IC.CASES[0]
    _, d, _, _ = _inputs(0)
    lib, h = _handle(c)
    eager = _memory(c)
    want = [_run(c, d, eager, slice(0, 4)), _run(c, d, eager, slice(4, 8))]
    mem = _memory(c)
    halves = [{k: v[f].contiguous() for k, v in d.items()} for f in (slice(0, 4), slice(4, 8))]
    x = {k: v.clone() for k, v in halves[0].items()}           # the graph's input buffers
    o = _outputs(c, 4, _capi.IDENT_FIELDS)
    idt = _struct(c, mem, o)
    side = torch.cuda.Stream()
    before = {k: v.clone() for k, v in mem.items()}
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    rc = lib.sqair_lane_identity_test(h, *[x[k].data_ptr() for k in INPUTS], 4, IC.B, C.byref(idt), ss)
    assert rc == 0, lib.sqair_last_error(h)
    assert lib.sqair_capture_end(h, ss, 3) == 1, lib.sqair_last_error(h)      # one launch: one kernel node
    torch.cuda.synchronize()
    for k, v in before.items():       # (a capture launches nothing: the memory is as it was)
        assert torch.equal(mem[k].view(torch.int32) if v.dtype == torch.float32 else mem[k], v.view(torch.int32) if v.dtype == torch.float32 else v), k
    for half, w in zip(halves, want):
        for k in x:
            x[k].copy_(half[k])
        torch.cuda.synchronize()
        assert lib.sqair_capture_launch(h, 3, ss) == 0, lib.sqair_last_error(h)
        torch.cuda.synchronize()
        for n in _capi.IDENT_FIELDS:
            assert np.array_equal(o[n].cpu().numpy(), w[n]), n
    for n in eager:
        a, b = eager[n], mem[n]
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), n
