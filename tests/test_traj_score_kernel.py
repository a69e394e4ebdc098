"""-m gpu: the trajectory scoring kernel (k_lane_traj_score, through sqair_lane_traj_score -- the entry takes caller tensors, so it is
its own kernel-level entry) against the float64 reference of tests/traj_score_ref.py, on the tables of tests/traj_score_cases.py:
210 lanes of F = 5 and 8 lanes of F = 300 (the grid's second chunk of frames), (G, N) = (4, 4), (1, 4) and (16, 14) on the wide
library, iou_min 0.5 and 0.3, with and without valid_mass and keep_id.

The integer outputs (``link``, ``state``, ``count_map``), ``counts`` and ``lane_counts`` are compared exactly on the lanes the
fragile rule does not leave out (tests/traj_score_ref.py: fragile_lanes; at most 1 % of the lanes, and tests/test_traj_score_ref.py
holds these inputs to none at all); ``link_iou``, ``p_alive``, ``pair_iou`` and ``centre_err`` within four times the error of an fp32
NumPy restatement against float64, measured on these very inputs from the reference alone (fp32_errors); ``sums`` within the bar
times the number of terms.  Also here: a second call exactly doubles ``counts``; a captured graph replayed twice equals two eager
calls bit for bit, ``sums`` included; an invalid-anchor lane's accumulators are untouched; the per-call outputs are optional.  With
SQAIR_PARITY_DIR set the measured figures are added to traj_score_parity.json there (the copy under profiles/ is such a file)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from tests import traj_score_cases as TC
from tests import traj_score_ref as R
from tests.abi_host import open_handle
from tests.kernel_unit import merge_parity

pytestmark = pytest.mark.gpu

IDS = [TC.case_id(c) for c in TC.CASES]


def _record(case, **figures):
    def update(data):
        data["build_id"] = _capi.build_id()
        data["device"] = torch.cuda.get_device_name(0)
        data["cases"].setdefault(case, {})["kernel"] = figures
    merge_parity("traj_score_parity.json", lambda: {"cases": {}}, update)


_handles = {}


def _handle(c):
    key = (c.wide, c.N)
    if key not in _handles:
        _handles[key] = open_handle(_capi.WIDE_LIB_PATH if c.wide else None, TC.HW, k_particles=TC.K, n_steps_per_image=c.N, n_what=6)
    return _handles[key]


@functools.lru_cache(maxsize=None)
def _inputs(i):
    """The case's inputs on the device, the reference, the bars and the lanes compared: made once, never written to."""
    c = TC.CASES[i]
    tab, tr, keep = TC.make(c)
    dev = {n: torch.from_numpy(np.array(v)).cuda() for n, v in list(tab.items()) + list(tr.items())}
    if keep is not None:
        dev["keep_id"] = torch.from_numpy(np.array(keep)).cuda()
    ref = R.score(tab, tr, c.iou_min, keep)
    bar = R.bars(R.fp32_errors(tab, tr, ref))
    whole = ~R.fragile_lanes(tab, tr, ref, c.iou_min, max(bar["link_iou"], bar["pair_iou"]))
    return tab, tr, dev, ref, bar, whole


def _state(c):
    z = lambda shp, dt: torch.zeros(shp, dtype=dt, device="cuda")
    return dict(counts=z((c.F, c.B, len(R.COUNTS)), torch.int64), sums=z((c.F, c.B, len(R.SUMS)), torch.float64),
                lane_counts=z((c.B, len(R.LANE_COUNTS)), torch.int64))


def _outputs(c, fields=_capi.TRAJ_FIELDS):
    shapes = _capi.traj_shapes(c.F, c.B, c.G)
    return {n: torch.full(shapes[n], -7, dtype=torch.int32 if n in _capi.TRAJ_INT_FIELDS else torch.float32, device="cuda") for n in fields}


def _launch(c, dev, state, out, stream=None):
    lib, h = _handle(c)
    tab = _capi.SqairLaneTraj(**{n: dev[n].data_ptr() for n in _capi.TRAJ_TABLE_FIELDS if n in dev})
    tru = _capi.SqairTrajTruth(G=c.G, **{n: dev[n].data_ptr() for n in _capi.TRAJ_TRUTH_FIELDS if n in dev})
    sco = _capi.SqairTrajScore(iou_min=c.iou_min, **{n: t.data_ptr() for n, t in state.items()}, **{n: t.data_ptr() for n, t in out.items()})
    s = stream or torch.cuda.current_stream()
    rc = lib.sqair_lane_traj_score(h, C.byref(tab), C.byref(tru), C.byref(sco), c.F, c.B, C.c_void_p(s.cuda_stream))
    assert rc == 0, lib.sqair_last_error(h)


def _run(c, dev, state, fields=_capi.TRAJ_FIELDS):
    out = _outputs(c, fields)
    _launch(c, dev, state, out)
    torch.cuda.synchronize()
    return {n: t.cpu().numpy() for n, t in out.items()}


@pytest.mark.parametrize("i", range(len(TC.CASES)), ids=IDS)
def test_kernel_against_fp64(i):
    c = TC.CASES[i]
    tab, tr, dev, ref, bar, whole = _inputs(i)
    state = _state(c)
    got = _run(c, dev, state)
    counts, sums, lane_counts = (state[n].cpu().numpy() for n in ("counts", "sums", "lane_counts"))
    left_out = int((~whole).sum())
    print(TC.case_id(c), "lanes left out as fragile:", left_out, "of", c.B)
    assert left_out <= TC.FRAGILE_CAP * c.B
    lanes = lambda n, a: a[whole] if n in ("link", "link_iou") else a[:, whole]      # ([B, G]; the others are [F, B, ...])
    for n in R.INT_OUT:
        assert got[n].dtype == np.int32 and np.array_equal(lanes(n, got[n]), lanes(n, getattr(ref, n))), (n, np.argwhere(got[n] != getattr(ref, n))[:4])
    assert np.array_equal(counts[:, whole], ref.counts[:, whole]), np.argwhere(counts != ref.counts)[:4]
    assert np.array_equal(lane_counts[whole], ref.lane_counts[whole]), np.argwhere(lane_counts != ref.lane_counts)[:4]
    err = {}
    for n in R.FLOAT_OUT:
        err[n] = float(lanes(n, np.abs(got[n].astype(np.float64) - getattr(ref, n))).max())
    # sums: within the bar times the number of terms
    terms = (ref.counts[..., 1], ref.counts[..., 1], ref.counts[..., 1] + ref.counts[..., 3] + ref.counts[..., 4])
    per_term = {}
    for k, (n, name) in enumerate(zip(R.SUMS, ("pair_iou", "centre_err", "brier"))):
        d = np.abs(sums[..., k] - ref.sums[..., k])
        assert (d <= bar[name] * terms[k])[:, whole].all(), (n, float(d.max()))
        per_term[n] = float((d / np.maximum(terms[k], 1))[:, whole].max())
    tot = dict(zip(R.COUNTS, counts.sum((0, 1)).tolist()))
    print(TC.case_id(c), "largest errors", {n: "{:.3g}".format(e) for n, e in err.items()}, "sums per term",
          {n: "{:.3g}".format(e) for n, e in per_term.items()}, "allowed", {n: "{:.3g}".format(e) for n, e in bar.items()}, tot)
    _record(TC.case_id(c), error=err, sums_per_term=per_term, allowed=bar, lanes=c.B, left_out=left_out, **tot)
    assert all(0.0 < bar[n] < 1e-5 for n in bar) and all(err[n] <= bar[n] for n in R.FLOAT_OUT), (err, bar)
    # lanes and frames that are not scored: -1 / 0, accumulators untouched
    nl, il = TC.nan_lane(c), TC.invalid_lane(c)
    off = ~R.frames_on(tab, tr)
    assert (got["state"][off] == -1).all() and (got["count_map"][off] == -1).all()
    assert not any(got[n][off].any() for n in ("p_alive", "pair_iou", "centre_err")) and not counts[off].any() and not sums[off].any()
    for lane in (nl, il):
        assert (got["link"][lane] == -1).all() and not got["link_iou"][lane].any()
    assert lane_counts[nl].tolist() == [0, 1, 0, 0] and not lane_counts[il].any()
    assert np.isfinite(sums).all() and min(tot.values()) > 0


@pytest.mark.parametrize("i", [1, 6, 7], ids=[IDS[i] for i in (1, 6, 7)])
def test_a_second_call_doubles_the_counts_and_a_replayed_graph_accumulates_the_bits_of_eager_calls(i):
    c = TC.CASES[i]
    tab, tr, dev, ref, _, _ = _inputs(i)
    il = TC.invalid_lane(c)
    eager = _state(c)
    eager["counts"][:, il].fill_(-3)           # the invalid-anchor lane's accumulators are untouched: whatever is there stays
    eager["lane_counts"][il].fill_(-3)
    eager["sums"][:, il].fill_(0.125)
    start = {n: t.clone() for n, t in eager.items()}
    first = _run(c, dev, eager)
    one = {n: t.clone() for n, t in eager.items()}
    second = _run(c, dev, eager)
    for n in _capi.TRAJ_FIELDS:               # the per-call outputs do not depend on the accumulators
        assert np.array_equal(first[n].view(np.int32), second[n].view(np.int32)), n
    for n in ("counts", "lane_counts"):
        assert torch.equal(eager[n] - start[n], 2 * (one[n] - start[n])), n
    keep = np.ones(c.B, bool)
    keep[il] = False
    assert np.array_equal((one["counts"] - start["counts"]).cpu().numpy()[:, keep], ref.counts[:, keep])
    assert torch.equal(eager["counts"][:, il], start["counts"][:, il]) and torch.equal(eager["lane_counts"][il], start["lane_counts"][il])
    assert torch.equal(eager["sums"][:, il], start["sums"][:, il])
    # a captured graph of the one launch (sqair_capture_begin / _end), replayed twice
    lib, h = _handle(c)
    graph_state = {n: t.clone() for n, t in start.items()}
    out = _outputs(c)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    ss = C.c_void_p(side.cuda_stream)
    assert lib.sqair_capture_begin(h, ss) == 0, lib.sqair_last_error(h)
    _launch(c, dev, graph_state, out, stream=side)
    assert lib.sqair_capture_end(h, ss, 3) == 1, lib.sqair_last_error(h)      # one launch per call: one kernel node
    torch.cuda.synchronize()
    for n, t in start.items():                # (the capture launched nothing)
        assert torch.equal(graph_state[n], t), n
    for _ in range(2):
        assert lib.sqair_capture_launch(h, 3, ss) == 0, lib.sqair_last_error(h)
    torch.cuda.synchronize()
    for n in graph_state:
        assert torch.equal(graph_state[n], eager[n]), n
    assert np.array_equal(graph_state["sums"].cpu().numpy().view(np.int64), eager["sums"].cpu().numpy().view(np.int64))
    for n in _capi.TRAJ_FIELDS:
        assert np.array_equal(out[n].cpu().numpy().view(np.int32), first[n].view(np.int32)), n


def test_the_per_call_outputs_are_optional():
    i = 1
    c = TC.CASES[i]
    _, _, dev, _, _, _ = _inputs(i)
    full_state = _state(c)
    full = _run(c, dev, full_state)
    for fields in ((), ("pair_iou",), ("link", "count_map"), ("state", "p_alive", "centre_err", "link_iou")):
        st = _state(c)
        part = _run(c, dev, st, fields=fields)
        assert all(np.array_equal(part[n].view(np.int32), full[n].view(np.int32)) for n in fields)
        assert all(torch.equal(full_state[n], st[n]) for n in st), fields
    # without obj_id (no keep) and with an all-ones valid_mass: the bits of the plain call
    j = 0
    c = TC.CASES[j]
    _, _, dev, _, _, _ = _inputs(j)
    a_state, b_state = _state(c), _state(c)
    a = _run(c, dev, a_state)
    other = dict(dev, valid_mass=torch.ones((c.F, c.B), device="cuda"))
    del other["obj_id"]
    b = _run(c, other, b_state)
    assert all(np.array_equal(a[n].view(np.int32), b[n].view(np.int32)) for n in a) and all(torch.equal(a_state[n], b_state[n]) for n in a_state)
