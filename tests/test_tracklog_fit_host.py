"""No GPU: the C-ABI of motion calibration (include/sqair_hip.h: sqair_lane_tracklog_fit) -- exported and declared in all three
libraries, the binding mirrors the header's struct and constants, the track log fit paragraph carries the semantics, every refusal of
the entry is made before any HIP call (dummy device pointers are enough) -- and the argument errors of ``track_log_fit`` and
``set_motion``."""
import ctypes as C
import os

import pytest

from sqair_amd import _capi
from sqair_amd.lane import LaneAnswers
from sqair_amd.stream import SqairStream
from tests.abi_host import (DUMMY, LIBS, ROOT, c_layout, constant, dummy, err as _err, fields as header_fields, handle, paragraph, phrases,
                            prototype, stated_once)

INF = float("inf")
NAN = float("nan")
N = 3
NAME = "sqair_lane_tracklog_fit"
COUNTS = ("n", "n_gap", "skipped")
SUMS = ("nis_sum", "lns_sum", "gap_nis_sum", "gap_lns_sum")


def _log(L=8, without=()):
    return dummy(_capi.SqairLaneTrackLog, 0xa000, _capi.TRACKLOG_FIELDS, without, L=L)


def _table(without=()):
    return dummy(_capi.SqairTrackLogOut, 0xb000, _capi.TRACKLOG_OUT_FIELDS, without)


def _fit(q=(0.25, 1.0), r=(1.0,), v0_var=16.0, burn=2, without=(), **more):
    ptr = {n: 0xd000 + 0x100 * i for i, n in enumerate(("counts", "sums", "innov")) if n not in without}
    f = _capi.tracklog_fit_struct(q, r, v0_var, burn, **ptr)
    for k, v in more.items():
        setattr(f, k, v)
    return f


def test_the_symbol_is_exported_and_declared_and_the_abi_is_unchanged(tmp_path):
    for path in (None, _capi.WIDE_LIB_PATH, _capi.TIMELINE_LIB_PATH):
        lib = _capi.lib(path)
        assert hasattr(lib, NAME) and lib.sqair_abi_version() == 2
    assert NAME in _capi.EXPORTED_SYMBOLS and _capi.ABI_VERSION == 2
    assert prototype(NAME) == (
        "int sqair_lane_tracklog_fit(SqairHandle* h, const SqairLaneTrackLog* log, const SqairTrackLogOut* table, const void* work, "
        "const SqairTrackLogFit* fit, int lag, int C, int N, int B, void* stream)")
    assert header_fields("SqairTrackLogFit") == [
        ("int32_t", "Q"), ("int32_t", "R"), ("int32_t", "burn"), ("float", "v0_var"), ("float[16]", "q"), ("float[16]", "r"),
        ("int64_t*", "counts"), ("double*", "sums"), ("float*", "innov")]
    assert [n for n, _ in _capi.SqairTrackLogFit._fields_] == ["Q", "R", "burn", "v0_var", "q", "r", "counts", "sums", "innov"]
    lay = c_layout(tmp_path, {"SqairTrackLogFit": ["Q", "R", "burn", "v0_var", "q", "r", "counts", "sums", "innov"]})
    offsets = [getattr(_capi.SqairTrackLogFit, n).offset for n in ("Q", "R", "burn", "v0_var", "q", "r", "counts", "sums", "innov")]
    assert lay["SqairTrackLogFit"] == (C.sizeof(_capi.SqairTrackLogFit), offsets) == (168, [0, 4, 8, 12, 16, 80, 144, 152, 160])
    assert constant("SQAIR_TRACKLOG_FIT_MAX_GRID") == 16 == _capi.TRACKLOG_FIT_MAX_GRID
    assert constant("SQAIR_TRACKLOG_FIT_COUNTS") == 3 and _capi.TRACKLOG_FIT_COUNTS == COUNTS
    assert constant("SQAIR_TRACKLOG_FIT_SUMS") == 4 and _capi.TRACKLOG_FIT_SUMS == SUMS
    assert _capi.TRACKLOG_FIT_TABLE == ("frame_index", "state") and _capi.TRACKLOG_FIT_REQUIRED == ("counts", "sums")
    assert _capi.field_dtype("SqairTrackLogFit", "counts") == "int64" and _capi.field_dtype("SqairTrackLogFit", "sums") == "float64"
    assert _capi.field_dtype("SqairTrackLogFit", "innov") == "float32"
    assert _capi.tracklog_fit_shapes(5, 2, 3, 4, 6) == dict(counts=(2, 4, 6, 3), sums=(2, 4, 6, 4), innov=(5, 2, 3, 2, 2))
    f = _capi.tracklog_fit_struct((0.5, 2.0), (1.0, 3.0, 9.0), 16.0, 1, counts=0x10, sums=0x20)
    assert (f.Q, f.R, f.burn, f.v0_var) == (2, 3, 1, 16.0) and list(f.q)[:3] == [0.5, 2.0, 0.0] and list(f.r)[:4] == [1.0, 3.0, 9.0, 0.0]
    assert (f.counts, f.sums, f.innov) == (0x10, 0x20, None)


def test_the_header_states_the_semantics_once():
    doc = paragraph("motion calibration: fit q and r to the track log", "#define SQAIR_TRACKLOG_FIT_MAX_GRID")
    phrases(doc, ("the track log fit paragraph", "-log p = 1/2 sum (ln 2 pi S + y y / S)", "the maximum-likelihood fit",
                  "is 1 per axis for an honest filter", "stand-alone, capturable call", "one launch of k_lane_tracklog_fit",
                  "it registers nothing", "no pass runs it", "it writes only its outputs", "nothing of them is read",
                  "The handle gives the error text only",
                  "`table` and `work` (both read-only) are what sqair_lane_tracklog_smooth wrote for the same lag, C, N and B",
                  "only frame_index and state are read", "the slot of every (frame, column)", "of `log`, L and log_box",
                  "A frame's record is frame_index mod L, as in the scorer", "No pass may have run between the solve and the fit",
                  "per lane b, per candidate (iq, ir) with (q, r) = (fit->q[iq], fit->r[ir]), per column c and per axis a in {y, x}",
                  "frames in ascending order, st = state[f,b,c]", "1. st 0 or 3: nothing happens", "2. The first st == 1",
                  "(p, v, Ppp, Ppv, Pvv) = (z, 0, r, 0, v0_var)", "z = fmaf(0.5, size, origin) of the slot's box words",
                  "exactly as in the solve's point 3", "i = 0, gap = false", "3. st == 2: P; gap = true", "4. A later st == 1",
                  "S = P's return; y = z - p; nis = (y * y) / S in fp32; i += 1",
                  "If i > burn, the term COUNTS when S > 0 and nis is finite", "n += 1, nis_sum += (double)nis",
                  "lns_sum += log((double)S)", "the logarithm taken in fp64, so that no fp32 logf enters the definition",
                  "n_gap, gap_nis_sum, gap_lns_sum when gap is set", "if i > burn and the term does not count, skipped += 1",
                  "Then U; gap = false", "innov[f,b,c,a,:] = (y, S) for candidate (0, 0) at these frames, whatever burn is",
                  "0 everywhere else", "5. The filter is sq_kf_predict and sq_kf_update", "called, not restated",
                  "adds its terms in frame order in fp64", "one thread then adds a candidate's 2 C partial sums in (c, a) index order",
                  "No float atomics", "a replayed graph gives the bits of an eager call", "Every word of every output is written",
                  "counts [B,Q,R,3] int64 = n, n_gap, skipped", "sums [B,Q,R,4] fp64 = nis_sum, lns_sum, gap_nis_sum, gap_lns_sum",
                  "1/2 (n ln 2 pi + lns_sum + nis_sum)", "The fit conditions on the associations the log recorded",
                  "it does not re-link objects", "Refused (return -1, text in sqair_last_error, before any HIP call)",
                  "a NULL log, table, work or fit", "what sqair_set_tracklog refuses for log", "a NULL frame_index or state of the table",
                  "a NULL counts or sums", "lag outside 1..L", "C outside 1..64", "N outside 1..16", "B < 1", "Q or R outside 1..16",
                  "burn < 0", "v0_var or any read q[i] / r[i] not finite and positive",
                  "Out of scope", "fitting v0_var or gate", "gradient or EM refinement inside a grid cell", "call again with a finer grid",
                  "per-track or per-lane scalars inside the identity kernel", "re-linking under the candidate scalars",
                  "the particles' spread as r", "filtering h, w", "sums that persist over windows", "training passes"))
    stated_once("motion calibration: fit q and r to the track log")
    assert constant("SQAIR_ABI_VERSION") == 2
    for name in ("DESIGN.md", "README.md"):
        text = " ".join(open(os.path.join(ROOT, name)).read().split())
        assert "sqair_lane_tracklog_fit" in text and "k_lane_tracklog_fit" in text and "track_log_fit" in text and "set_motion" in text, name


@pytest.mark.parametrize("path", LIBS)
def test_the_entrys_refusals_before_any_hip_call(path):
    with handle(path, k_particles=2, n_steps_per_image=N) as (lib, h):
        good = dict(log=_log(L=8), table=_table(), work=DUMMY, fit=_fit(), lag=8, C=4, N=N, B=2)

        def call(**kw):
            a = dict(good, **kw)
            ref = lambda v: C.byref(v) if v is not None else None
            return lib.sqair_lane_tracklog_fit(h, ref(a["log"]), ref(a["table"]), a["work"], ref(a["fit"]), a["lag"], a["C"], a["N"], a["B"],
                                               DUMMY)
        assert lib.sqair_lane_tracklog_fit(None, C.byref(good["log"]), C.byref(good["table"]), DUMMY, C.byref(good["fit"]), 8, 4, N, 2,
                                           DUMMY) == -1
        for kw in (dict(log=None), dict(table=None), dict(work=None), dict(fit=None)):
            assert call(**kw) == -1 and "sqair_lane_tracklog_fit: log, table, work and fit must not be NULL" in _err(lib, h), kw
        for L in (0, 4097):                                                             # what sqair_set_tracklog refuses for the log
            assert call(log=_log(L=L)) == -1 and "L = {} must lie in 1..4096".format(L) in _err(lib, h)
        for missing in _capi.TRACKLOG_FIELDS:
            assert call(log=_log(without=(missing,))) == -1 and "count, log_valid, log_id, log_len and log_box must not be NULL" in _err(lib, h)
        for lag in (0, -1, 9, 4097):
            assert call(lag=lag) == -1 and "sqair_lane_tracklog_fit: lag" in _err(lib, h) and "must lie in 1..L" in _err(lib, h), lag
        for Cn in (0, -1, 65):
            assert call(C=Cn) == -1 and "C must lie in 1..64" in _err(lib, h)
        for n in (0, -1, 17):
            assert call(N=n) == -1 and "N must lie in 1..16" in _err(lib, h)
        for b in (0, -3):
            assert call(B=b) == -1 and "B = {} must be >= 1".format(b) in _err(lib, h)
        for kw in (dict(Q=0), dict(Q=17), dict(Q=-1), dict(R=0), dict(R=17)):
            assert call(fit=_fit(**kw)) == -1 and "must lie in 1..16" in _err(lib, h) and "Q = " in _err(lib, h), kw
        for burn in (-1, -100):
            assert call(fit=_fit(burn=burn)) == -1 and "burn = {} must be >= 0".format(burn) in _err(lib, h)
        for bad in (0.0, -1.0, INF, NAN):
            assert call(fit=_fit(v0_var=bad)) == -1 and "v0_var must be finite and > 0" in _err(lib, h), bad
            assert call(fit=_fit(q=(0.25, bad))) == -1 and "q[1] must be finite and > 0" in _err(lib, h), bad
            assert call(fit=_fit(r=(bad,))) == -1 and "r[0] must be finite and > 0" in _err(lib, h), bad
        for missing in ("frame_index", "state"):
            assert call(table=_table(without=(missing,))) == -1 and "frame_index and state must not be NULL" in _err(lib, h)
        for missing in ("counts", "sums"):
            assert call(fit=_fit(without=(missing,))) == -1 and "counts and sums must not be NULL" in _err(lib, h)


def _answers(motion=False, tracklog=8, **kw):
    base = ("SqairStream", True, 0.5, False, False, 0.5)
    rest = (True, 0.3, None, 10, 4.0, INF, True, "row")
    return LaneAnswers(*base, False, 0.5, None, *rest, motion=motion, tracklog=tracklog, tracklog_tracks=4, **kw)


def test_track_log_fit_argument_errors():
    """The arguments are checked before the core is touched (these objects have none)."""
    with pytest.raises(ValueError, match=r"^SqairStream.track_log_fit: the stream keeps no track log"):
        _answers(tracklog=None).track_log_fit()
    la = _answers()
    for bad in (0, -1, 9, 2.0, True, "4"):
        with pytest.raises(ValueError, match=r"^SqairStream.track_log_fit: lag must be an integer in \[1, tracklog = 8\]"):
            la.track_log_fit(lag=bad)
    for name in ("q_grid", "r_grid"):
        for bad in ((), [], [1.0] * 17, "abc", 3.0):
            with pytest.raises(ValueError, match=r"^SqairStream.track_log_fit: {} must hold 1 to 16 values".format(name)):
                la.track_log_fit(**{name: bad})
        for bad in ((1.0, 0.0), (-1.0,), (INF,), (1.0, NAN)):
            with pytest.raises(ValueError, match=r"^SqairStream.track_log_fit: every value of {} must be finite and > 0".format(name)):
                la.track_log_fit(**{name: bad})
    for bad in (-1, 1.0, True, "2", None):
        with pytest.raises(ValueError, match=r"^SqairStream.track_log_fit: burn must be an integer >= 0"):
            la.track_log_fit(burn=bad)
    for bad in (0.0, -2.0, INF, NAN):
        with pytest.raises(ValueError, match=r"^SqairStream.track_log_fit: v0 must be finite and > 0"):
            la.track_log_fit(v0=bad)
    assert la._check_grid("q_grid", None, 0.25) == [0.25 * 4.0 ** k for k in range(-4, 4)] and la._check_grid("q_grid", None, 0.25)[4] == 0.25
    assert hasattr(SqairStream, "track_log_fit") and hasattr(SqairStream, "set_motion")


def test_set_motion_argument_errors_and_defaults():
    la = _answers()
    for name in ("q", "r", "v0", "gate"):
        for bad in (0.0, -1.0, INF, NAN, "x"):
            with pytest.raises(ValueError, match=r"^SqairStream.set_motion: {} must be finite and > 0".format(name)):
                la.set_motion(**{name: bad})
    assert la.motion_scalars == dict(q=0.25, r=1.0, v0_var=16.0, gate=3.0)               # a refused call changes nothing
    assert la.set_motion(q=1.0, r=0.25) is False                                        # (no motion on this stream: only the defaults)
    assert la.motion_scalars == dict(q=1.0, r=0.25, v0_var=16.0, gate=3.0)
    assert la.set_motion(v0=4.0, gate=2.0) is False and la.motion_scalars == dict(q=1.0, r=0.25, v0_var=4.0, gate=2.0)
    assert la._check_log_call("track_log", None, None, None, None) == (8, dict(q=1.0, r=0.25, v0=4.0))
    assert la._check_grid("r_grid", None, la.motion_scalars["r"])[4] == 0.25
