"""No GPU: the C-ABI of trajectory scoring (include/sqair_hip.h: sqair_lane_traj_score) -- exported and declared, the binding mirrors
the header's three structs, the header's paragraph carries the semantics once, every refusal is made before any HIP call (dummy
device pointers are enough) -- and the argument errors of SqairStream.forecast / tracks(truth=...) and trajectory_score()."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.lane import TrajScores
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, constant, dummy, err as _err, fields as header_fields, handle, paragraph, prototype,
                            stated_once)

TABLE_NEEDED = tuple(n for n in _capi.TRAJ_TABLE_FIELDS if n not in _capi.TRAJ_TABLE_OPTIONAL)
TRUTH_NEEDED = tuple(n for n in _capi.TRAJ_TRUTH_FIELDS if n != "keep_id")


def _table(without=()):
    return dummy(_capi.SqairLaneTraj, 0x2000, _capi.TRAJ_TABLE_FIELDS, without)


def _truth(G=4, without=("keep_id",)):
    return dummy(_capi.SqairTrajTruth, 0x4000, _capi.TRAJ_TRUTH_FIELDS, without, G=G)


def _score(iou_min=0.5, without=()):
    return dummy(_capi.SqairTrajScore, 0x6000, _capi.TRAJ_ACCUMULATORS + _capi.TRAJ_FIELDS, without, iou_min=iou_min)


def test_the_symbol_is_exported_and_declared_and_the_abi_is_unchanged():
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, "sqair_lane_traj_score") and lib.sqair_abi_version() == 2
        assert not hasattr(lib, "sqair_lane_traj_score_test")      # the entry takes caller tensors: it is its own kernel-level entry
    assert "sqair_lane_traj_score" in _capi.EXPORTED_SYMBOLS
    assert prototype("sqair_lane_traj_score") == ("int sqair_lane_traj_score(SqairHandle* h, const SqairLaneTraj* table, "
                                                  "const SqairTrajTruth* truth, const SqairTrajScore* score, int F, int B, void* stream)")
    assert _capi.ABI_VERSION == 2 == constant("SQAIR_ABI_VERSION")
    assert constant("SQAIR_TRAJ_COUNTS") == len(_capi.TRAJ_COUNTS)
    assert constant("SQAIR_TRAJ_SUMS") == len(_capi.TRAJ_SUMS)
    assert constant("SQAIR_TRAJ_LANE_COUNTS") == len(_capi.TRAJ_LANE_COUNTS)
    # the binding's structs mirror the header's, field for field and in order
    tab, tru, sco = (header_fields(n) for n in ("SqairLaneTraj", "SqairTrajTruth", "SqairTrajScore"))
    assert [n for _, n in tab] == [n for n, _ in _capi.SqairLaneTraj._fields_] == list(_capi.TRAJ_TABLE_FIELDS)
    assert [n for _, n in tru] == [n for n, _ in _capi.SqairTrajTruth._fields_] == ["G"] + list(_capi.TRAJ_TRUTH_FIELDS)
    assert [n for _, n in sco] == [n for n, _ in _capi.SqairTrajScore._fields_] == ["iou_min"] + list(_capi.TRAJ_ACCUMULATORS + _capi.TRAJ_FIELDS)
    assert all(ty.startswith("const ") and ty.endswith("*") for ty, _ in tab)          # the table is read-only
    assert [n for ty, n in tab if ty == "const int32_t*"] == ["best_row"]
    assert all(ty.startswith("const ") for ty, n in tru if n != "G") and dict((n, ty) for ty, n in tru)["G"] == "int32_t"
    assert [n for ty, n in tru if ty == "const int32_t*"] == ["anchor_present", "anchor_valid", "truth_present", "truth_valid", "keep_id"]
    types_ = {n: ty for ty, n in sco}
    assert types_["counts"] == "int64_t*" and types_["sums"] == "double*" and types_["lane_counts"] == "int64_t*" and types_["iou_min"] == "float"
    assert [n for ty, n in sco if ty == "int32_t*"] == list(_capi.TRAJ_INT_FIELDS)
    assert C.sizeof(_capi.SqairLaneTraj) == 8 * 9 and C.sizeof(_capi.SqairTrajTruth) == 8 + 8 * 7 and C.sizeof(_capi.SqairTrajScore) == 8 + 8 * 10
    assert _capi.traj_shapes(2, 3, 5) == dict(link=(3, 5), link_iou=(3, 5), state=(2, 3, 5), p_alive=(2, 3, 5), pair_iou=(2, 3, 5),
                                              centre_err=(2, 3, 5), count_map=(2, 3))
    # the shared fields are fields of both tables
    shared = [n for n in _capi.TRAJ_TABLE_FIELDS if n != "valid_mass"]
    assert all(n in _capi.FORECAST_LANE_FIELDS and n in _capi.TRACK_LANE_FIELDS for n in shared) and "valid_mass" in _capi.TRACK_LANE_FIELDS
    # the counters' order is the header's
    doc = paragraph()
    assert "counts[f,b,:] int64 = (frames, pairs, hits, lost, gone, count_hit, count_abs_err)" in doc
    assert "fp64 = (iou_sum, centre_err_sum, brier_sum)" in doc
    assert "lane_counts[b,:] += (calls, calls_invalid, anchor_truth, linked)" in doc
    assert _capi.TRAJ_COUNTS == ("frames", "pairs", "hits", "lost", "gone", "count_hit", "count_abs_err")
    assert _capi.TRAJ_SUMS == ("iou_sum", "centre_err_sum", "brier_sum")
    assert _capi.TRAJ_LANE_COUNTS == ("calls", "calls_invalid", "anchor_truth", "linked")


def test_the_header_states_the_semantics_once():
    doc = paragraph("trajectory scoring: a lane forecast or a lane track table", "#define SQAIR_TRAJ_COUNTS")
    once = ("k_lane_traj_score", "neither registered on the handle nor part of a pass", "after sqair_forecast_fan or sqair_history_trace_lane",
            "The handle gives N and the error text only", "it is its own kernel-level entry", "NULL: mass 1 everywhere",
            "the last stepped frame (frame F-1 of lane tracks, the frame before f = 0 of a forecast)", "Lane not scored",
            "anchor_valid[b] == 0: the lane is untouched", "best_row[b] == -1", "counts one calls_invalid and changes nothing else",
            "Link, once per call", "sq_box_iou(anchor_box[b,g], box0[b,j])", "sq_assign_keep_greedy, the score's device function, unchanged",
            "link[b,g] = j or -1", "truth_valid[f,b] != 0 and valid_mass[f,b] > 0", "a NULL valid_mass counts as positive",
            "p = alive[f,b,j] / support[b,j], an fp32 division", "brier = (p - y)^2", "state 1, a pair", "state 2, lost", "state 0, gone",
            "a NaN box_mean is never read", "(y + h/2, x + w/2)", "hits += [pair_iou >= iou_min]", "Only the Brier term counts",
            "state[f,b,g] = -1 and zeros", "the first argmax of count_prob[f,b,:]", "linked or not", "count_hit += [count_map == n_truth]",
            "count_abs_err += |count_map - n_truth|", "g in index order", "one thread owns each cell (f, b)", "no float atomics",
            "a replayed graph accumulates the bits eager calls do", "before any HIP call", "F outside 1..65535 or B < 1", "G outside 1..16",
            "iou_min NaN or outside (0, 1]", "a keep_id without a table obj_id", "Out of scope", "optimal (Hungarian) assignment",
            "calibration of box_std", "trajectory scoring per particle row", "truth for departed objects", "a truth ring kept by the stream")
    shared = ("g in index order", "no float atomics", "before any HIP call", "G outside 1..16", "iou_min NaN or outside (0, 1]",
              "Out of scope", "optimal (Hungarian) assignment")      # other paragraphs say these of their own kernels
    flat = paragraph()
    for word in once:
        assert doc.count(word) == 1, word
        assert word in shared or flat.count(word) == 1, word         # stated in this paragraph and nowhere else
    assert "truth identity IS the slot g" in doc
    stated_once("trajectory scoring: a lane forecast or a lane track table")
    # the score's paragraph is as it was, a pointer follows it
    assert "scoring of forecasts or lane tracks; training passes. */" in flat
    assert "Forecasts and lane tracks are scored by sqair_lane_traj_score" in flat
    for name in ("DESIGN.md", "README.md", os.path.join("tools", "README.md")):      # they point to the header, they do not restate it
        text = open(os.path.join(ROOT, name)).read()
        assert ("sqair_lane_traj_score" in text or "traj_score_time" in text), name
        assert "an fp32 division" not in text and "state 2, lost" not in text, name


@pytest.mark.parametrize("path", LIBS)
def test_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=3) as (lib, h):
        good = dict(table=_table(), truth=_truth(), score=_score(), F=5, B=3)

        def call(**kw):
            a = dict(good, **kw)
            ref = lambda s: None if s is None else C.byref(s)
            return lib.sqair_lane_traj_score(h, ref(a["table"]), ref(a["truth"]), ref(a["score"]), a["F"], a["B"], DUMMY)
        assert lib.sqair_lane_traj_score(None, C.byref(good["table"]), C.byref(good["truth"]), C.byref(good["score"]), 5, 3, DUMMY) == -1
        for kw in (dict(table=None), dict(truth=None), dict(score=None)):
            assert call(**kw) == -1 and "sqair_lane_traj_score" in _err(lib, h) and "must not be NULL" in _err(lib, h), kw
        for missing in TABLE_NEEDED:
            assert call(table=_table(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h) and missing in _err(lib, h), missing
        for missing in TRUTH_NEEDED:
            assert call(truth=_truth(without=("keep_id", missing))) == -1 and "must not be NULL" in _err(lib, h) and missing in _err(lib, h)
        for missing in _capi.TRAJ_ACCUMULATORS:
            assert call(score=_score(without=(missing,))) == -1 and "must not be NULL" in _err(lib, h) and missing in _err(lib, h)
        for F in (0, -1, 65536):
            assert call(F=F) == -1 and "F = {}".format(F) in _err(lib, h) and "1..65535" in _err(lib, h)
        for B in (0, -2):
            assert call(B=B) == -1 and "B = {}".format(B) in _err(lib, h)
        for bad in (0, -1, 17, 1 << 20):
            assert call(truth=_truth(G=bad)) == -1 and "must lie in 1..16" in _err(lib, h), bad
        for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
            assert call(score=_score(iou_min=bad)) == -1 and "iou_min must lie in (0, 1]" in _err(lib, h), bad
        assert call(table=_table(without=("obj_id",)), truth=_truth(without=())) == -1 and "keep_id needs the table's obj_id" in _err(lib, h)


# ---- the stream's argument errors: all raised before the core is touched -------------------------------------------------------------
def _stream(scored=False, G=0, B=3, K=2, T=1):
    """A stream's argument checks without a device: the attributes they read, and a core and a carried state that fail when touched."""
    st = SqairStream.__new__(SqairStream)
    st.B, st.K, st.T, st.R = B, K, T, B * K
    st.core = types.SimpleNamespace(N=3)
    st.carried = types.SimpleNamespace(ring=object(), history=8)
    st.lane = types.SimpleNamespace(scored=scored, G=G)
    st.traj = TrajScores(st.core, B, st.lane)
    return st


def _truth_dict(F, B=3, G=2, anchor=True, **kw):
    t = dict(box=np.zeros((F, B, G, 4), np.float32), present=np.ones((F, B, G), np.int32))
    if anchor:
        t.update(anchor_box=np.zeros((B, G, 4), np.float32), anchor_present=np.ones((B, G), np.int32))
    t.update(kw)
    return t


def test_stream_argument_errors():
    st = _stream()
    fc = lambda **kw: st.forecast(4, samples=2, **kw)
    tk = lambda **kw: st.tracks(6, **kw)
    for call, name, F in ((fc, "forecast", 4), (tk, "tracks", 6)):
        who = r"^SqairStream\.{}: ".format(name)
        with pytest.raises(ValueError, match=who + "truth is for a call with lane=True"):
            call(truth=_truth_dict(F))
        with pytest.raises(ValueError, match=who + "truth must be a dict with box, present"):
            call(lane=True, truth=dict(box=np.zeros((F, 3, 2, 4))))
        with pytest.raises(ValueError, match=who + "truth must be a dict with box, present"):
            call(lane=True, truth=_truth_dict(F, boxes=1))
        for bad in (0.0, 1.5, float("nan")):
            with pytest.raises(ValueError, match=who + r"truth_iou must lie in \(0, 1\]"):
                call(lane=True, truth=_truth_dict(F), truth_iou=bad)
        # wrong shapes, each named
        with pytest.raises(ValueError, match=who + r"truth\['box'\] of shape \({}, 3, 2, 4\) given, \[{}, 3, 2, 4\] expected".format(F + 1, F)):
            call(lane=True, truth=_truth_dict(F, box=np.zeros((F + 1, 3, 2, 4), np.float32)))
        with pytest.raises(ValueError, match=who + r"truth\['box'\] of shape .* with G in \[1, 16\] expected"):
            call(lane=True, truth=_truth_dict(F, G=17))
        with pytest.raises(ValueError, match=who + r"truth\['box'\] of shape"):
            call(lane=True, truth=_truth_dict(F, box=np.zeros((F, 3, 2), np.float32)))
        with pytest.raises(ValueError, match=who + r"truth\['present'\] of shape \({}, 3, 3\) given".format(F)):
            call(lane=True, truth=_truth_dict(F, present=np.ones((F, 3, 3), np.int32)))
        with pytest.raises(ValueError, match=who + r"truth\['valid'\] of shape \(3,\) given, \[{}, 3\] expected".format(F)):
            call(lane=True, truth=_truth_dict(F, valid=np.ones(3, np.int32)))
        with pytest.raises(ValueError, match=who + r"truth\['anchor_box'\] of shape \(3, 3, 4\) given, \[3, 2, 4\] expected"):
            call(lane=True, truth=_truth_dict(F, anchor_box=np.zeros((3, 3, 4), np.float32)))
        with pytest.raises(ValueError, match=who + r"truth\['anchor_present'\] of shape"):
            call(lane=True, truth=_truth_dict(F, anchor_present=np.ones((3, 1), np.int32)))
        with pytest.raises(ValueError, match=who + r"truth\['anchor_valid'\] of shape \(2,\) given, \[3\] expected"):
            call(lane=True, truth=_truth_dict(F, anchor_valid=np.ones(2, np.int32)))
        with pytest.raises(ValueError, match=who + r"truth\['anchor_box'\] and truth\['anchor_present'\] come together"):
            call(lane=True, truth=_truth_dict(F, anchor=False, anchor_box=np.zeros((3, 2, 4), np.float32)))
        # link_ids: a scored stream of the same G, and a call with truth
        with pytest.raises(ValueError, match=who + "link_ids is for a stream with score=True and the same G"):
            call(lane=True, truth=_truth_dict(F), link_ids=True)
        with pytest.raises(ValueError, match=who + "link_ids is for a call with truth"):
            call(lane=True, link_ids=True)
    with pytest.raises(ValueError, match=r"^SqairStream\.forecast: a forecast's truth needs anchor_box and anchor_present"):
        fc(lane=True, truth=_truth_dict(4, anchor=False))
    other = _stream(scored=True, G=3)
    with pytest.raises(ValueError, match="link_ids is for a stream with score=True and the same G"):
        other.forecast(4, lane=True, truth=_truth_dict(4, G=2), link_ids=True)
    # trajectory_score
    with pytest.raises(ValueError, match=r"^SqairStream\.trajectory_score: kind must be 'forecast' or 'tracks'"):
        st.trajectory_score("future")
    for kind in ("forecast", "tracks"):
        with pytest.raises(ValueError, match=r"^SqairStream\.trajectory_score: no {} call has been scored yet".format(kind)):
            st.trajectory_score(kind)


def test_the_checked_truth_is_in_the_abis_names_and_dtypes():
    st = _stream()
    fn = "SqairStream.tracks: "
    t = st._check_traj_truth(fn, _truth_dict(6, anchor=False, present=np.ones((6, 3, 2), bool)), True, 6, True, False, 0.4)
    assert t["G"] == 2 and abs(t["iou_min"] - 0.4) < 1e-12 and set(t) == {"G", "iou_min"} | set(TRUTH_NEEDED)
    assert t["truth_box"].dtype == torch.float32 and all(t[n].dtype == torch.int32 for n in TRUTH_NEEDED if "box" not in n)
    assert tuple(t["anchor_box"].shape) == (3, 2, 4) and tuple(t["anchor_present"].shape) == (3, 2) and bool(t["anchor_valid"].all())
    # a trace's anchor defaults to its newest frame, anchor_valid to that frame's valid
    box = np.arange(6 * 3 * 2 * 4, dtype=np.float32).reshape(6, 3, 2, 4)
    valid = np.ones((6, 3), np.int32)
    valid[5, 1] = 0
    t = st._check_traj_truth(fn, dict(box=box, present=np.ones((6, 3, 2), np.int32), valid=valid), True, 6, True, False, 0.5)
    assert np.array_equal(t["anchor_box"].numpy(), box[5]) and t["anchor_valid"].tolist() == [1, 0, 1]
    assert st._check_traj_truth(fn, None, False, 6, True, False, 0.5) is None
