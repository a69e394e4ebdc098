"""ctypes binding of libsqair_hip.so, made from the C header at import: include/sqair_hip.h is the one statement of the C-ABI
(sqair_amd/_abi.py parses it), so the header travels with the package and an import without it fails.  What is written here is what
the header does not state in code: the shapes, which fields of a struct are inputs and which outputs, the column names of the counter
tables, the names a step's ``lane`` dict uses.

The library is built in-tree by ``__graft_entry__.build()`` / ``sqair_amd/csrc/build.py``.  There is
no CPU fallback: if the shared object is missing the import of the HIP path fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

from sqair_amd import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsqair_hip.so")

_HEADER = _abi.header()
_K = _HEADER.constants
# SqairLogprobTest.out: the address of a SqairOutputs, set as an integer like the device addresses beside it
_STRUCTS, _HEADER_PROTOS = _abi.bind(_HEADER, addresses={("SqairLogprobTest", "out")})
globals().update(_STRUCTS)   # SqairConfig, SqairOutputs, SqairSmc, ...: one ctypes.Structure per struct of the header
field_dtype = _abi.field_dtype


def _pointers(struct, after=None, without=()):
    """The pointer fields of a struct in declaration order (``after``: those behind that field), but for ``without``."""
    names = [f.name for f in _HEADER.structs[struct] if f.pointer_depth]
    return tuple(n for n in names[names.index(after) + 1 if after else 0:] if n not in without)


def _int32(struct, names):
    """Those of the struct's fields ``names`` that the header types int32_t*."""
    return tuple(n for n in names if field_dtype(struct, n) == "int32")


def _counted(constant, *names):
    """The column names of a counter table, as many as the header's constant says."""
    assert len(names) == _K[constant], "{} is {} in the header, this binding names {} columns".format(constant, _K[constant], len(names))
    return names


OUTPUT_FIELDS = [f.name for f in _HEADER.structs["SqairOutputs"]]
N_REFERENCE_OUTPUTS = 38  # the TensorArrays of reference sqair/seq.py:121-177

# object forecasts (include/sqair_hip.h: sqair_forecast_fan): the outputs of SqairForecastLane in declaration order, with their shapes
# in terms of F, B, K, N (R = B * K)
FORECAST_LANE_FIELDS = _pointers("SqairForecastLane")
FORECAST_LANE_INT_FIELDS = _int32("SqairForecastLane", FORECAST_LANE_FIELDS)
FORECAST_FAN_MAX = _K["SQAIR_FORECAST_FAN_MAX"]


def forecast_lane_shapes(F, B, K, N):
    R = B * K
    return dict(best_row=(B,), weights=(B, K), start_where=(R, N, 4), start_presence=(R, N), start_obj_id=(R, N), obj_id=(B, N),
                presence=(B, N), box0=(B, N, 4), support=(B, N), alive=(F, B, N), box_mean=(F, B, N, 4), box_std=(F, B, N, 4),
                count_prob=(F, B, N + 1))


# lane estimates (include/sqair_hip.h: sqair_set_estimate): the outputs of SqairLaneEstimate in declaration order; the int32 ones
ESTIMATE_FIELDS = _pointers("SqairLaneEstimate", after="log_w")
ESTIMATE_INT_FIELDS = _int32("SqairLaneEstimate", ESTIMATE_FIELDS)


def estimate_shapes(T, B, K, N, nw, canvas_hw=None):
    """The outputs' shapes for passes of T frames; ``canvas_hw``: (H, W) when mean_canvas is asked for."""
    shapes = dict(best_row=(T, B), weights=(T, B, K), ess=(T, B), count_prob=(T, B, N + 1), expected_count=(T, B), map_count=(T, B),
                  presence=(T, B, N), obj_id=(T, B, N), where=(T, B, N, 4), what=(T, B, N, nw), box=(T, B, N, 4), support=(T, B, N),
                  box_mean=(T, B, N, 4))
    if canvas_hw is not None:
        shapes["mean_canvas"] = (T, B) + tuple(canvas_hw)
    return shapes


# object layers (include/sqair_hip.h: sqair_set_layers): the outputs of SqairLaneLayers in declaration order; the int32 ones
LAYERS_FIELDS = _pointers("SqairLaneLayers")
LAYERS_INT_FIELDS = _int32("SqairLaneLayers", LAYERS_FIELDS)


def layers_shapes(T, B, K, N, hw):
    """The outputs' shapes for passes of T frames over frames of ``hw`` = (H, W)."""
    hw = tuple(hw)
    return dict(match=(T, B, K, N), layer=(T, B, N) + hw, cover=(T, B, N) + hw, owner=(T, B) + hw)


# stream scoring (include/sqair_hip.h: sqair_set_score): the inputs and accumulators of SqairLaneScore; the per-frame outputs, the
# rest of its pointers, and the int32 ones among them; the columns of ``counts``
SCORE_INPUTS = ("truth_box", "truth_present", "truth_valid", "counts", "iou_sum", "last_id")
SCORE_FIELDS = _pointers("SqairLaneScore", without=SCORE_INPUTS)
SCORE_INT_FIELDS = _int32("SqairLaneScore", SCORE_FIELDS)
SCORE_COUNTS = _counted("SQAIR_SCORE_COUNTS", "frames", "frames_invalid", "truth", "tp", "fn", "fp", "idsw", "count_hit", "count_abs_err")
SCORE_MAX_TRUTH = _K["SQAIR_SCORE_MAX_TRUTH"]


def score_shapes(T, B, G):
    """The per-frame outputs' shapes for passes of T frames and G truth slots per lane."""
    return dict(truth_match=(T, B, G), match_iou=(T, B, G), tp=(T, B), fn=(T, B), fp=(T, B), idsw=(T, B))


# IDF1 scoring (include/sqair_hip.h: sqair_set_idf): the table's fields of SqairLaneIdf in declaration order with their shapes, then
# ``totals`` and its columns -- the twelve figures of a clip
IDF_TABLE = _pointers("SqairLaneIdf", without=("totals",))
IDF_TOTALS = _counted("SQAIR_IDF_TOTALS", "clips", "frames", "trajectories", "idtp", "idfn", "idfp", "mt", "pt", "ml", "frag", "ids",
                      "overflow_ids")
IDF_MAX_IDS = _K["SQAIR_IDF_MAX_IDS"]


def idf_shapes(B, G, P):
    """The table's shapes for G truth slots and P id columns per lane, and ``totals``."""
    return dict(col_id=(B, P), overlap=(B, G, P), row_frames=(B, G), col_frames=(B, P), extra_frames=(B,), matched=(B, G), frag=(B, G),
                trk_state=(B, G), frames=(B,), totals=(B, len(IDF_TOTALS)))


# HOTA scoring (include/sqair_hip.h: sqair_set_hota): the log's fields of SqairLaneHota in declaration order (the column table, the
# records, the counters and the solve's scratch), then the three totals and their columns; the solve's optional outputs
HOTA_TOTALS = ("totals_i", "totals_f", "totals_c")
HOTA_LOG = _pointers("SqairLaneHota", without=HOTA_TOTALS)
HOTA_INT = ("tp", "fn", "fp", "loc")
HOTA_FLOAT = ("ass", "assre", "asspr")
HOTA_CLIP = ("clips", "frames", "dropped_frames", "overflow_ids")
HOTA_ALPHAS = _K["SQAIR_HOTA_ALPHAS"]
HOTA_MAX_IDS = _K["SQAIR_HOTA_MAX_IDS"]
HOTA_MAX_FRAMES = _K["SQAIR_HOTA_MAX_FRAMES"]
HOTA_BINS = HOTA_ALPHAS + 1


def hota_shapes(B, G, N, P, L):
    """The log's shapes for G truth slots, N object slots, P id columns and L records per lane, and the totals."""
    return dict(col_id=(B, P), log_q=(B, L, G, N), log_col=(B, L, N), log_row=(B, L), frames=(B,), dropped_frames=(B,),
                work=(B, G, P, HOTA_BINS), totals_i=(B, HOTA_ALPHAS, len(HOTA_INT)), totals_f=(B, HOTA_ALPHAS, len(HOTA_FLOAT)),
                totals_c=(B, len(HOTA_CLIP)))


def hota_solve_shapes(B, G, L):
    """The shapes of sqair_lane_hota_solve's optional outputs, and of its mask."""
    return dict(open_i=(B, HOTA_ALPHAS, len(HOTA_INT)), open_f=(B, HOTA_ALPHAS, len(HOTA_FLOAT)), open_c=(B, len(HOTA_CLIP)),
                match=(B, L, G), close=(B,))


# lane identities (include/sqair_hip.h: sqair_set_identity): the names the per-frame outputs of SqairLaneIdentity have in a step's
# ``lane`` dict; the scalars before them and the memory, the rest of its pointers; the columns of ``counts``
IDENT_LANE_NAMES = dict(lane_id="lane_id", how="id_how", track_len="track_len")
IDENT_FIELDS = tuple(IDENT_LANE_NAMES)
IDENT_INT_FIELDS = _int32("SqairLaneIdentity", IDENT_FIELDS)
IDENT_SCALARS = tuple((n, t) for n, t in _STRUCTS["SqairLaneIdentity"]._fields_ if t is not C.c_void_p)
IDENT_MEMORY = _pointers("SqairLaneIdentity", without=IDENT_FIELDS)
IDENT_COUNTS = _counted("SQAIR_IDENT_COUNTS", "frames", "frames_invalid", "objects", "kept", "bridged", "reidentified", "born", "ended")
IDENT_MAX_TRACKS = _K["SQAIR_IDENT_MAX_TRACKS"]


def identity_shapes(T, B, N):
    """The per-frame outputs' shapes for passes of T frames, by their names in a step's ``lane`` dict."""
    return {IDENT_LANE_NAMES[n]: (T, B, N) for n in IDENT_FIELDS}


def identity_memory_shapes(B, M, nw):
    """The memory's and the counters' shapes for M track entries per lane."""
    return dict(trk_id=(B, M), trk_word=(B, M), trk_age=(B, M), trk_len=(B, M), trk_box=(B, M, 4), trk_what=(B, M, nw), next_id=(B,),
                counts=(B, len(IDENT_COUNTS)))


# lane motion (include/sqair_hip.h: sqair_set_motion): the scalars of SqairLaneMotion, its state and its per-frame outputs, which
# keep their names in a step's ``lane`` dict; the five words of the state per (entry, axis)
MOTION_SCALARS = tuple(n for n, t in _STRUCTS["SqairLaneMotion"]._fields_ if t is not C.c_void_p)
MOTION_MEMORY = ("trk_kf",)
MOTION_FIELDS = _pointers("SqairLaneMotion", without=MOTION_MEMORY)
MOTION_STATE = ("p", "v", "Ppp", "Ppv", "Pvv")


def motion_shapes(T, B, N):
    """The per-frame outputs' shapes for passes of T frames."""
    return dict(velocity=(T, B, N, 2), nis=(T, B, N))


def motion_memory_shapes(B, M):
    """The filter state's shape for M track entries per lane: (y, x) x MOTION_STATE."""
    return dict(trk_kf=(B, M, 2, len(MOTION_STATE)))


# the track log (include/sqair_hip.h: sqair_set_tracklog): the fields of SqairLaneTrackLog -- the counter and the records -- and the
# outputs of the solve in declaration order, with the int32 ones among them (frame_index is int64); the four values of ``state``
TRACKLOG_FIELDS = _pointers("SqairLaneTrackLog")
TRACKLOG_OUT_FIELDS = _pointers("SqairTrackLogOut")
TRACKLOG_OUT_INT_FIELDS = _int32("SqairTrackLogOut", TRACKLOG_OUT_FIELDS)
TRACKLOG_MAX_FRAMES = _K["SQAIR_TRACKLOG_MAX_FRAMES"]
TRACKLOG_MAX_TRACKS = _K["SQAIR_TRACKLOG_MAX_TRACKS"]
TRACKLOG_STATES = ("outside", "seen", "gap", "invalid")


def tracklog_shapes(B, L, N):
    """The log's shapes for L records per lane and N object slots."""
    return dict(count=(B,), log_valid=(B, L), log_id=(B, L, N), log_len=(B, L, N), log_box=(B, L, N, 4))


def tracklog_out_shapes(lag, B, C):
    """The shapes of sqair_lane_tracklog_smooth's outputs for a window of ``lag`` frames and C track columns."""
    return dict(track_id=(B, C), n_tracks=(B,), len0=(B, C), frame_index=(lag, B), state=(lag, B, C), size=(lag, B, C, 2),
                filt=(lag, B, C, 2, len(MOTION_STATE)), smooth=(lag, B, C, 2, len(MOTION_STATE)))


# track log scoring (include/sqair_hip.h: sqair_lane_tracklog_score): the truth's pointer fields, the score's required outputs and its
# optional ones with the int32 ones among them, the four views by name, the columns of ``counts`` [B, 4, .] and ``sums`` [B, 4, .]
TRACKLOG_TRUTH_FIELDS = _pointers("SqairTrackLogTruth")
TRACKLOG_SCORE_TABLE = ("track_id", "frame_index", "state", "size", "filt", "smooth")   # what the scorer reads of the solve's outputs
TRACKLOG_SCORE_REQUIRED = ("counts", "sums")
TRACKLOG_SCORE_FIELDS = _pointers("SqairTrackLogScore", without=TRACKLOG_SCORE_REQUIRED)
TRACKLOG_SCORE_INT_FIELDS = _int32("SqairTrackLogScore", TRACKLOG_SCORE_FIELDS)
TRACKLOG_SCORE_VIEWS = _counted("SQAIR_TRACKLOG_SCORE_VIEWS", "filtered", "smooth", "filtered_filled", "smooth_filled")
TRACKLOG_SCORE_COUNTS = _counted("SQAIR_TRACKLOG_SCORE_COUNTS", "frames", "frames_invalid", "truth", "tp", "fn", "fp", "idsw", "gap_tp",
                                 "gap_fp", "nees_n", "gap_nees_n", "idtp", "idfn", "idfp")
TRACKLOG_SCORE_SUMS = _counted("SQAIR_TRACKLOG_SCORE_SUMS", "iou_sum", "err_sum", "nees_sum", "gap_err_sum", "gap_nees_sum")


def tracklog_truth_shapes(lag, B, G):
    """The truth's shapes for a window of ``lag`` frames and G truth slots per lane (window order)."""
    return dict(truth_box=(lag, B, G, 4), truth_present=(lag, B, G), truth_valid=(lag, B))


def tracklog_score_shapes(lag, B, G):
    """The shapes of sqair_lane_tracklog_score's outputs, required and optional."""
    V = len(TRACKLOG_SCORE_VIEWS)
    return dict(counts=(B, V, len(TRACKLOG_SCORE_COUNTS)), sums=(B, V, len(TRACKLOG_SCORE_SUMS)), assign=(V, B, G), match=(V, lag, B, G),
                match_iou=(V, lag, B, G))


# motion calibration (include/sqair_hip.h: sqair_lane_tracklog_fit): what the fit reads of the solve's outputs, its required outputs,
# the longest grid, the columns of ``counts`` [B, Q, R, .] and ``sums`` [B, Q, R, .]
TRACKLOG_FIT_TABLE = ("frame_index", "state")
TRACKLOG_FIT_REQUIRED = ("counts", "sums")
TRACKLOG_FIT_MAX_GRID = _K["SQAIR_TRACKLOG_FIT_MAX_GRID"]
TRACKLOG_FIT_COUNTS = _counted("SQAIR_TRACKLOG_FIT_COUNTS", "n", "n_gap", "skipped")
TRACKLOG_FIT_SUMS = _counted("SQAIR_TRACKLOG_FIT_SUMS", "nis_sum", "lns_sum", "gap_nis_sum", "gap_lns_sum")


def tracklog_fit_shapes(lag, B, C, Q, R):
    """The shapes of sqair_lane_tracklog_fit's outputs, required and optional, for a Q x R grid of candidates."""
    return dict(counts=(B, Q, R, len(TRACKLOG_FIT_COUNTS)), sums=(B, Q, R, len(TRACKLOG_FIT_SUMS)), innov=(lag, B, C, 2, 2))


def tracklog_fit_struct(q_grid, r_grid, v0_var, burn, **pointers):
    """A SqairTrackLogFit for the grids given as sequences of floats; ``pointers``: counts, sums and optionally innov (addresses)."""
    fit = _STRUCTS["SqairTrackLogFit"](Q=len(q_grid), R=len(r_grid), burn=burn, v0_var=v0_var, **pointers)
    for i, v in enumerate(q_grid):
        fit.q[i] = v
    for i, v in enumerate(r_grid):
        fit.r[i] = v
    return fit


# track log stitching (include/sqair_hip.h: sqair_lane_tracklog_stitch): the link outputs in declaration order, the result's names for
# them, what the stitch reads of the solve's outputs
TRACKLOG_STITCH_FIELDS = _pointers("SqairTrackLogStitch")
TRACKLOG_STITCH_LINKS = dict(zip(("next", "d2", "gap", "root", "n_links"), TRACKLOG_STITCH_FIELDS))
TRACKLOG_STITCH_TABLE = ("track_id", "n_tracks", "len0", "frame_index", "state", "filt", "smooth")


def tracklog_stitch_shapes(B, C):
    """The shapes of sqair_lane_tracklog_stitch's link outputs for C track columns."""
    return dict(link_next=(B, C), link_d2=(B, C), link_gap=(B, C), root=(B, C), n_links=(B,))


# trajectory scoring (include/sqair_hip.h: sqair_lane_traj_score): the three structs' pointer fields in declaration order -- of
# SqairTrajScore the accumulators, then the per-call outputs and the int32 ones among them --, the columns of ``counts`` [F, B, .],
# ``sums`` [F, B, .] and ``lane_counts`` [B, .]
TRAJ_TABLE_FIELDS = _pointers("SqairLaneTraj")
TRAJ_TABLE_OPTIONAL = ("obj_id", "valid_mass")
TRAJ_TRUTH_FIELDS = _pointers("SqairTrajTruth")
TRAJ_ACCUMULATORS = ("counts", "sums", "lane_counts")
TRAJ_FIELDS = _pointers("SqairTrajScore", without=TRAJ_ACCUMULATORS)
TRAJ_INT_FIELDS = _int32("SqairTrajScore", TRAJ_FIELDS)
TRAJ_COUNTS = _counted("SQAIR_TRAJ_COUNTS", "frames", "pairs", "hits", "lost", "gone", "count_hit", "count_abs_err")
TRAJ_SUMS = _counted("SQAIR_TRAJ_SUMS", "iou_sum", "centre_err_sum", "brier_sum")
TRAJ_LANE_COUNTS = _counted("SQAIR_TRAJ_LANE_COUNTS", "calls", "calls_invalid", "anchor_truth", "linked")


def traj_shapes(F, B, G):
    """The per-call outputs' shapes for a table of F frames and G truth slots per lane."""
    return dict(link=(B, G), link_iou=(B, G), state=(F, B, G), p_alive=(F, B, G), pair_iou=(F, B, G), centre_err=(F, B, G),
                count_map=(F, B))


# track history (include/sqair_hip.h: sqair_set_history): the bit of each output a ring slot may hold; the first three are mandatory
HISTORY_FIELDS = {n: _K["SQAIR_HIST_" + bit] for n, bit in (("where", "WHERE"), ("presence", "PRESENCE"), ("obj_id", "OBJ_ID"),
                                                            ("what", "WHAT"), ("log_weights_per_timestep", "LOG_W"))}
HISTORY_MANDATORY = ("where", "presence", "obj_id")
assert sum(HISTORY_FIELDS[n] for n in HISTORY_MANDATORY) == _K["SQAIR_HIST_MANDATORY"] and sum(HISTORY_FIELDS.values()) == _K["SQAIR_HIST_ALL"]
TRACE_FIELDS = _pointers("SqairTraceOutputs")

# lane tracks (include/sqair_hip.h: sqair_history_trace_lane): the outputs of SqairTraceLane in declaration order, with their shapes
# in terms of F = lag * T, B, K, N
TRACK_LANE_FIELDS = _pointers("SqairTraceLane")
TRACK_LANE_INT_FIELDS = _int32("SqairTraceLane", TRACK_LANE_FIELDS)


def track_lane_shapes(F, B, K, N):
    return dict(best_row=(B,), weights=(B, K), obj_id=(B, N), presence=(B, N), box0=(B, N, 4), support=(B, N), first_frame=(B, N),
                alive=(F, B, N), box_mean=(F, B, N, 4), box_std=(F, B, N, 4), count_prob=(F, B, N + 1), valid_mass=(F, B))


# sqair_debug_dense_routes: the families of the two dense launchers, in the order include/sqair_hip.h documents
DENSE_ROUTES = _counted("SQAIR_DENSE_ROUTES", "fwd_splitk", "fwd_t2", "fwd_rows", "fwd_mt", "fwd_lds", "fwd_big_2x2", "fwd_big_3x2",
                        "fwd_big_3x3", "fwd_big_4x2", "dx_nch1", "dx_nch2", "dx_nch3", "dx_nch4", "dx_nch5", "dx_nch6", "dx_nch7", "dx_nch8",
                        "dx_nch9", "dx_nch12", "dx_nch18", "dx_t2", "dx_gru1", "dx_gru2", "fwd_strip")


def dense_routes(library=None):
    """{family: launches of it this process has issued or captured so far} for the two dense launchers."""
    v = (C.c_int64 * len(DENSE_ROUTES))()
    n = (library or lib()).sqair_debug_dense_routes(v, len(DENSE_ROUTES))
    assert n == len(DENSE_ROUTES), "the library counts {} dense routes, this binding names {}".format(n, len(DENSE_ROUTES))
    return dict(zip(DENSE_ROUTES, (int(x) for x in v)))


# what include/sqair_hip.h declares: everything but the measurement helpers -- and the one read-out among them that it documents
EXPORTED_SYMBOLS = list(_HEADER_PROTOS)
# the measurement helpers the header deliberately does not declare, typed by hand
_PROTOS = dict(_HEADER_PROTOS, **{
    "sqair_debug_linear_time": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                          C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_float), C.c_void_p]),
    "sqair_debug_linear_graph_time": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                              C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_void_p]),
    "sqair_debug_dense_log": (C.c_int, [C.c_void_p, C.c_int]),
    "sqair_debug_dense_log_entry": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "sqair_debug_specialised_launches": (C.c_int64, []),
    "sqair_debug_wgrad_launches": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sqair_debug_layers": (C.c_int, [C.c_void_p]),
    "sqair_debug_padded_count": (C.c_int64, [C.c_void_p, C.POINTER(C.c_int)]),
    "sqair_debug_layer": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                    C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sqair_debug_plan": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                   C.POINTER(C.c_int)]),
    "sqair_debug_plan_t": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
})

TIMELINE_LIB_PATH = os.path.join(_HERE, "libsqair_hip_timeline.so")
# the same sources compiled with -DSQAIR_WIDE: the rest of the reference's flag range (n_what up to 128, up to 16 object slots,
# n_units up to 16) on a larger slot record and plain-loop per-row kernels; same C-ABI, slower
WIDE_LIB_PATH = os.path.join(_HERE, "libsqair_hip_wide.so")
# what the product library is laid out for (csrc/sqair_glue.h: SQ_MAXN, SQ_MAX_NWHAT, SQ_MAX_NHIDDEN)
PRODUCT_LIMITS = dict(n_what=50, n_steps_per_image=8, n_hidden=256)
WIDE_LIMITS = dict(n_what=128, n_steps_per_image=14, n_hidden=512)   # (15, 16 slots: the log-probability adjoint's LDS staging does not fit the wide record)


def lib_path_for(n_what, n_steps_per_image, n_hidden):
    """The library a configuration runs on: the product library inside its limits, the wide build beyond them."""
    inside = (n_what <= PRODUCT_LIMITS["n_what"] and n_steps_per_image <= PRODUCT_LIMITS["n_steps_per_image"] and
              n_hidden <= PRODUCT_LIMITS["n_hidden"])
    return LIB_PATH if inside else WIDE_LIB_PATH

ABI_VERSION = _K["SQAIR_ABI_VERSION"]
_VARIANT_OF = {"libsqair_hip.so": "product", "libsqair_hip_timeline.so": "timeline", "libsqair_hip_knobs.so": "knobs",
               "libsqair_hip_wide.so": "wide"}

_libs = {}


class StaleLibraryError(ImportError):
    """The shared object was not compiled from the sources beside it."""


def source_id():
    """Hash of the kernel sources ON DISK (sqair_amd/csrc/ + include/sqair_hip.h + compiler flags): what a fresh build of any
    variant would report as its `sqair_build_id()`."""
    from .csrc import build as _b
    if not any(f.endswith(".hip") for f in os.listdir(_b.HERE)):
        raise OSError("no kernel sources in {}".format(_b.HERE))   # (build.py alone does not make a source tree)
    return _b.source_id()


def lib(path=None, allow_stale=False):
    """Loads the shared library (once per path).  Raises ImportError with the build hint if it is absent, if its ABI version is
    not this binding's, or (StaleLibraryError) if the build id compiled into it is not the hash of the sources on disk -- a
    binary is git-ignored and travels beside the sources, so nothing else ties the two together.  `path` selects a build
    VARIANT of the same sources (TIMELINE_LIB_PATH: every wave stamps its start / end, measurement only); the default is the
    product library.  There is no environment override."""
    path = path or LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise ImportError(
                "{} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` or "
                "`python sqair_amd/csrc/build.py [--timeline]`; sqair_amd has no CPU fallback".format(path))
        # torch first: its wheel bundles its own HIP runtime; loading ours before it would put two runtimes into the
        # process (the second one then reports "no ROCm-capable device")
        import torch  # noqa: F401
        l = C.CDLL(path)
        # the version first, through the one symbol every version has: a binding that has drifted fails HERE, not in a getattr
        l.sqair_abi_version.restype = C.c_int
        if l.sqair_abi_version() != ABI_VERSION:
            raise ImportError("{}: ABI version {} but this binding speaks {}; rebuild (python sqair_amd/csrc/build.py)".format(
                os.path.basename(path), l.sqair_abi_version(), ABI_VERSION))
        for name, (res, args) in _PROTOS.items():
            if allow_stale and not hasattr(l, name):
                continue   # (tools/ab_libs.py: a build of an older revision has the same ABI version but may lack a newer entry point)
            fn = getattr(l, name)
            fn.restype = res
            fn.argtypes = args
        got = l.sqair_build_id().decode()
        try:
            want = source_id()
        except (OSError, ImportError):   # a binary-only deployment (no csrc/ -- ModuleNotFoundError -- or its .hip files stripped; the
            # header is there, or this module would not have imported): nothing to compare with
            want = None
            if not allow_stale:
                import warnings
                warnings.warn("{}: the kernel sources are not beside the package, the staleness check of the binary "
                              "(build id {}) is skipped".format(os.path.basename(path), got))
        if want is not None and got != want and not allow_stale:
            raise StaleLibraryError(
                "{} was compiled from sources {} but the sources on disk are {}: rebuild (python sqair_amd/csrc/build.py "
                "--force [--timeline] [--knobs]); numbers measured on a stale binary would be attributed to the wrong "
                "code".format(os.path.basename(path), got, want))
        variant = _VARIANT_OF.get(os.path.basename(path))
        if variant is not None and l.sqair_build_flags().decode() != variant:
            raise ImportError("{} reports build variant '{}', expected '{}'".format(
                os.path.basename(path), l.sqair_build_flags().decode(), variant))
        _libs[path] = l
    return _libs[path]


def build_id(path=None):
    """The build id COMPILED INTO the loaded library (`sqair_build_id()`: the hash of the sources that binary was built from).
    Profiles carry it so that a number is only ever quoted next to the binary it was measured on; `lib()` has already checked
    that it equals `source_id()`."""
    return lib(path).sqair_build_id().decode()


def check(handle, rc, what, library=None):
    """Raises RuntimeError with the handle's error text.  `library` must be the shared object the handle came from (a handle of
    the timeline / knob variant is not the product library's to read): SqairCore.check passes its own."""
    if rc != 0:
        msg = (library or lib()).sqair_last_error(handle)
        raise RuntimeError("{} failed (rc={}): {}".format(what, rc, msg.decode() if msg else ""))
