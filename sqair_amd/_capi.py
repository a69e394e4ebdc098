"""ctypes binding of libsqair_hip.so (C-ABI declared in include/sqair_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``sqair_amd/csrc/build.py``.  There is
no CPU fallback: if the shared object is missing the import of the HIP path fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsqair_hip.so")

OUTPUT_FIELDS = [
    "what", "what_loc", "what_scale", "where", "where_loc", "where_scale", "presence_prob", "presence",
    "presence_logit", "obj_id", "step_log_prob", "canvas", "glimpse", "disc_what_log_prob",
    "disc_where_log_prob", "disc_what_prior_log_prob", "disc_where_prior_log_prob", "disc_log_prob",
    "disc_prior_log_prob", "disc_prob", "prop_what_log_prob", "prop_where_log_prob",
    "prop_what_prior_log_prob", "prop_where_prior_log_prob", "prop_log_prob", "prop_prior_log_prob",
    "prop_prob", "discrete_log_prob", "num_prop_steps_per_sample", "num_disc_steps_per_sample",
    "num_steps_per_sample", "prop_pres", "disc_pres", "data_ll_per_sample", "kl_per_sample",
    "log_q_z_given_x_per_sample", "log_p_z_per_sample", "log_weights_per_timestep",
    "final_temporal_state", "final_prior_state", "final_last_used_id",
]
N_REFERENCE_OUTPUTS = 38  # the TensorArrays of reference sqair/seq.py:121-177


class SqairConfig(C.Structure):
    _fields_ = [
        ("img_h", C.c_int32), ("img_w", C.c_int32), ("glimpse_size", C.c_int32),
        ("n_steps_per_image", C.c_int32), ("n_what", C.c_int32), ("n_hidden", C.c_int32),
        ("k_particles", C.c_int32), ("prop_prior_type", C.c_int32), ("disc_prior_type", C.c_int32),
        ("masked_glimpse", C.c_int32), ("rec_where_prior", C.c_int32),
        ("prop_prior_step_bias", C.c_float), ("step_success_prob", C.c_float), ("output_std", C.c_float),
        ("background_std", C.c_float), ("where_prior_mean", C.c_float * 4),
        ("sample_from_prior", C.c_int32), ("generate_after", C.c_int32), ("time_cell", C.c_int32), ("prior_cell", C.c_int32), ("rnn_cell", C.c_int32),
    ]


class SqairOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in OUTPUT_FIELDS]


class SqairSmc(C.Structure):
    """SMC resampling of a carried state (include/sqair_hip.h: sqair_set_smc); every pointer is a device address."""
    _fields_ = [
        ("ess_frac", C.c_float), ("seed", C.c_uint64), ("uniforms", C.c_void_p), ("log_w", C.c_void_p), ("log_z", C.c_void_p),
        ("log_evidence", C.c_void_p), ("ess", C.c_void_p), ("u_out", C.c_void_p), ("resampled", C.c_void_p),
        ("src_rows", C.c_void_p),
    ]


class SqairCarry(C.Structure):
    """A carried training chunk (include/sqair_hip.h: sqair_forward_train_carry / sqair_backward_carry); device addresses."""
    _fields_ = [
        ("state_in", C.c_void_p), ("state_out", C.c_void_p), ("src_rows", C.c_void_p), ("state_bytes", C.c_int64),
        ("B", C.c_int32), ("smc", C.POINTER(SqairSmc)),
    ]


class SqairForecastOutputs(C.Structure):
    """Outputs of sqair_forecast (include/sqair_hip.h); every pointer is a device address or None."""
    _fields_ = [(n, C.c_void_p) for n in ("what", "where", "presence", "presence_prob", "presence_logit", "obj_id", "canvas", "glimpse",
                                          "log_w", "mean_canvas", "expected_count")]


# object forecasts (include/sqair_hip.h: sqair_forecast_fan): the outputs of SqairForecastLane in declaration order, with their shapes
# in terms of F, B, K, N (R = B * K)
FORECAST_LANE_FIELDS = ("best_row", "weights", "start_where", "start_presence", "start_obj_id", "obj_id", "presence", "box0", "support",
                        "alive", "box_mean", "box_std", "count_prob")
FORECAST_LANE_INT_FIELDS = ("best_row",)
FORECAST_FAN_MAX = 1024


def forecast_lane_shapes(F, B, K, N):
    R = B * K
    return dict(best_row=(B,), weights=(B, K), start_where=(R, N, 4), start_presence=(R, N), start_obj_id=(R, N), obj_id=(B, N),
                presence=(B, N), box0=(B, N, 4), support=(B, N), alive=(F, B, N), box_mean=(F, B, N, 4), box_std=(F, B, N, 4),
                count_prob=(F, B, N + 1))


class SqairForecastLane(C.Structure):
    """One predictive answer per object of a lane from its K * S rollouts (include/sqair_hip.h: sqair_forecast_fan); every pointer is
    a device address, all but best_row optional."""
    _fields_ = [("iou_min", C.c_float)] + [(n, C.c_void_p) for n in FORECAST_LANE_FIELDS]


# lane estimates (include/sqair_hip.h: sqair_set_estimate): the outputs of SqairLaneEstimate in declaration order; the two int32 ones
ESTIMATE_FIELDS = ("best_row", "weights", "ess", "count_prob", "expected_count", "map_count", "presence", "obj_id", "where", "what",
                   "box", "support", "box_mean", "mean_canvas")
ESTIMATE_INT_FIELDS = ("best_row", "map_count")


def estimate_shapes(T, B, K, N, nw, canvas_hw=None):
    """The outputs' shapes for passes of T frames; ``canvas_hw``: (H, W) when mean_canvas is asked for."""
    shapes = dict(best_row=(T, B), weights=(T, B, K), ess=(T, B), count_prob=(T, B, N + 1), expected_count=(T, B), map_count=(T, B),
                  presence=(T, B, N), obj_id=(T, B, N), where=(T, B, N, 4), what=(T, B, N, nw), box=(T, B, N, 4), support=(T, B, N),
                  box_mean=(T, B, N, 4))
    if canvas_hw is not None:
        shapes["mean_canvas"] = (T, B) + tuple(canvas_hw)
    return shapes


class SqairLaneEstimate(C.Structure):
    """One answer per lane from its particles (include/sqair_hip.h: sqair_set_estimate); every pointer is a device address, all but
    best_row optional."""
    _fields_ = [("iou_min", C.c_float), ("log_w", C.c_void_p)] + [(n, C.c_void_p) for n in ESTIMATE_FIELDS]


# object layers (include/sqair_hip.h: sqair_set_layers): the outputs of SqairLaneLayers in declaration order; the two int32 ones
LAYERS_FIELDS = ("match", "layer", "cover", "owner")
LAYERS_INT_FIELDS = ("match", "owner")


def layers_shapes(T, B, K, N, hw):
    """The outputs' shapes for passes of T frames over frames of ``hw`` = (H, W)."""
    hw = tuple(hw)
    return dict(match=(T, B, K, N), layer=(T, B, N) + hw, cover=(T, B, N) + hw, owner=(T, B) + hw)


class SqairLaneLayers(C.Structure):
    """Per-object appearance, coverage and pixel owners of a lane (include/sqair_hip.h: sqair_set_layers); every pointer is a
    device address, each optional, at least one set."""
    _fields_ = [("cover_min", C.c_float)] + [(n, C.c_void_p) for n in LAYERS_FIELDS]


# stream scoring (include/sqair_hip.h: sqair_set_score): the per-frame outputs of SqairLaneScore in declaration order and the int32
# ones among them; the inputs and accumulators before them; the columns of ``counts``
SCORE_FIELDS = ("truth_match", "match_iou", "tp", "fn", "fp", "idsw")
SCORE_INT_FIELDS = ("truth_match", "tp", "fn", "fp", "idsw")
SCORE_INPUTS = ("truth_box", "truth_present", "truth_valid", "counts", "iou_sum", "last_id")
SCORE_COUNTS = ("frames", "frames_invalid", "truth", "tp", "fn", "fp", "idsw", "count_hit", "count_abs_err")
SCORE_MAX_TRUTH = 16


def score_shapes(T, B, G):
    """The per-frame outputs' shapes for passes of T frames and G truth slots per lane."""
    return dict(truth_match=(T, B, G), match_iou=(T, B, G), tp=(T, B), fn=(T, B), fp=(T, B), idsw=(T, B))


class SqairLaneScore(C.Structure):
    """CLEAR-MOT scoring of the lane answer against ground-truth boxes (include/sqair_hip.h: sqair_set_score); every pointer is a
    device address, the per-frame outputs (SCORE_FIELDS) optional."""
    _fields_ = [("iou_min", C.c_float), ("G", C.c_int32)] + [(n, C.c_void_p) for n in SCORE_INPUTS + SCORE_FIELDS]


# IDF1 scoring (include/sqair_hip.h: sqair_set_idf): the table's fields of SqairLaneIdf in declaration order (all int32) with their
# shapes, then ``totals`` (int64) and its columns -- the twelve figures of a clip
IDF_TABLE = ("col_id", "overlap", "row_frames", "col_frames", "extra_frames", "matched", "frag", "trk_state", "frames")
IDF_TOTALS = ("clips", "frames", "trajectories", "idtp", "idfn", "idfp", "mt", "pt", "ml", "frag", "ids", "overflow_ids")
IDF_MAX_IDS = 64


def idf_shapes(B, G, P):
    """The table's shapes for G truth slots and P id columns per lane (int32), and ``totals`` (int64)."""
    return dict(col_id=(B, P), overlap=(B, G, P), row_frames=(B, G), col_frames=(B, P), extra_frames=(B,), matched=(B, G), frag=(B, G),
                trk_state=(B, G), frames=(B,), totals=(B, len(IDF_TOTALS)))


class SqairLaneIdf(C.Structure):
    """The identity overlap table of a clip per lane and the totals over closed clips (include/sqair_hip.h: sqair_set_idf); every
    pointer is a device address, none optional."""
    _fields_ = [("P", C.c_int32)] + [(n, C.c_void_p) for n in IDF_TABLE + ("totals",)]


# lane identities (include/sqair_hip.h: sqair_set_identity): the scalars, the memory and the per-frame outputs of SqairLaneIdentity
# in declaration order (all outputs int32); the names the outputs have in a step's ``lane`` dict; the columns of ``counts``
IDENT_SCALARS = (("iou_min", C.c_float), ("reid_dist", C.c_float), ("reid_what", C.c_float), ("M", C.c_int32), ("max_age", C.c_int32))
IDENT_MEMORY = ("trk_id", "trk_word", "trk_age", "trk_len", "trk_box", "trk_what", "next_id", "counts")
IDENT_FIELDS = ("lane_id", "how", "track_len")
IDENT_LANE_NAMES = dict(lane_id="lane_id", how="id_how", track_len="track_len")
IDENT_COUNTS = ("frames", "frames_invalid", "objects", "kept", "bridged", "reidentified", "born", "ended")
IDENT_MAX_TRACKS = 16


def identity_shapes(T, B, N):
    """The per-frame outputs' shapes for passes of T frames, by their names in a step's ``lane`` dict."""
    return {IDENT_LANE_NAMES[n]: (T, B, N) for n in IDENT_FIELDS}


def identity_memory_shapes(B, M, nw):
    """The memory's and the counters' shapes for M track entries per lane; every array int32 but trk_box, trk_what (float32) and
    counts (int64)."""
    return dict(trk_id=(B, M), trk_word=(B, M), trk_age=(B, M), trk_len=(B, M), trk_box=(B, M, 4), trk_what=(B, M, nw), next_id=(B,),
                counts=(B, len(IDENT_COUNTS)))


class SqairLaneIdentity(C.Structure):
    """Stable per-lane track ids (include/sqair_hip.h: sqair_set_identity); every pointer is a device address, trk_what, how and
    track_len optional."""
    _fields_ = list(IDENT_SCALARS) + [(n, C.c_void_p) for n in IDENT_MEMORY + IDENT_FIELDS]


# trajectory scoring (include/sqair_hip.h: sqair_lane_traj_score): the three structs' pointer fields in declaration order, the int32
# ones among the per-call outputs, the columns of ``counts`` [F, B, .], ``sums`` [F, B, .] and ``lane_counts`` [B, .]
TRAJ_TABLE_FIELDS = ("best_row", "presence", "obj_id", "support", "box0", "alive", "box_mean", "count_prob", "valid_mass")
TRAJ_TABLE_OPTIONAL = ("obj_id", "valid_mass")
TRAJ_TRUTH_FIELDS = ("anchor_box", "anchor_present", "anchor_valid", "truth_box", "truth_present", "truth_valid", "keep_id")
TRAJ_ACCUMULATORS = ("counts", "sums", "lane_counts")
TRAJ_FIELDS = ("link", "link_iou", "state", "p_alive", "pair_iou", "centre_err", "count_map")
TRAJ_INT_FIELDS = ("link", "state", "count_map")
TRAJ_COUNTS = ("frames", "pairs", "hits", "lost", "gone", "count_hit", "count_abs_err")
TRAJ_SUMS = ("iou_sum", "centre_err_sum", "brier_sum")
TRAJ_LANE_COUNTS = ("calls", "calls_invalid", "anchor_truth", "linked")


def traj_shapes(F, B, G):
    """The per-call outputs' shapes for a table of F frames and G truth slots per lane."""
    return dict(link=(B, G), link_iou=(B, G), state=(F, B, G), p_alive=(F, B, G), pair_iou=(F, B, G), centre_err=(F, B, G),
                count_map=(F, B))


class SqairLaneTraj(C.Structure):
    """The table a lane forecast or a lane trace wrote, as the trajectory score reads it (include/sqair_hip.h:
    sqair_lane_traj_score); device addresses, obj_id and valid_mass optional."""
    _fields_ = [(n, C.c_void_p) for n in TRAJ_TABLE_FIELDS]


class SqairTrajTruth(C.Structure):
    """The truth of a trajectory score: the anchor and the table's frames; device addresses, keep_id optional."""
    _fields_ = [("G", C.c_int32)] + [(n, C.c_void_p) for n in TRAJ_TRUTH_FIELDS]


class SqairTrajScore(C.Structure):
    """The accumulators (required) and the per-call outputs (TRAJ_FIELDS, optional) of a trajectory score; device addresses."""
    _fields_ = [("iou_min", C.c_float)] + [(n, C.c_void_p) for n in TRAJ_ACCUMULATORS + TRAJ_FIELDS]


# track history (include/sqair_hip.h: sqair_set_history): the bit of each field a ring slot may hold; the first three are mandatory
HISTORY_FIELDS = {"where": 1, "presence": 2, "obj_id": 4, "what": 8, "log_weights_per_timestep": 16}
HISTORY_MANDATORY = ("where", "presence", "obj_id")
TRACE_FIELDS = ("where", "presence", "obj_id", "what", "log_w", "valid", "frame_index", "ancestor_row", "unique_ancestors", "track_id",
                "n_tracks", "track_present", "track_where")


class SqairTraceOutputs(C.Structure):
    """Outputs of sqair_history_trace (include/sqair_hip.h); T = frames per pass, every pointer a device address or None."""
    _fields_ = [("T", C.c_int32), ("max_tracks", C.c_int32)] + [(n, C.c_void_p) for n in TRACE_FIELDS]


# lane tracks (include/sqair_hip.h: sqair_history_trace_lane): the outputs of SqairTraceLane in declaration order, with their shapes
# in terms of F = lag * T, B, K, N
TRACK_LANE_FIELDS = ("best_row", "weights", "obj_id", "presence", "box0", "support", "first_frame", "alive", "box_mean", "box_std",
                     "count_prob", "valid_mass")
TRACK_LANE_INT_FIELDS = ("best_row", "first_frame")


def track_lane_shapes(F, B, K, N):
    return dict(best_row=(B,), weights=(B, K), obj_id=(B, N), presence=(B, N), box0=(B, N, 4), support=(B, N), first_frame=(B, N),
                alive=(F, B, N), box_mean=(F, B, N, 4), box_std=(F, B, N, 4), count_prob=(F, B, N + 1), valid_mass=(F, B))


class SqairTraceLane(C.Structure):
    """One smoothed trajectory per object of a lane from its K traced paths (include/sqair_hip.h: sqair_history_trace_lane); every
    pointer is a device address, all but best_row optional."""
    _fields_ = [("iou_min", C.c_float)] + [(n, C.c_void_p) for n in TRACK_LANE_FIELDS]


class SqairDenseSeg(C.Structure):
    _fields_ = [("p", C.c_void_p), ("ld", C.c_int32), ("width", C.c_int32), ("rdiv", C.c_int32)]


class SqairDenseContract(C.Structure):
    """One dense launch with everything the operand contract can say (include/sqair_hip.h: sqair_linear_contract_test); device
    addresses, handed to the launcher unchanged."""
    _fields_ = [("nseg", C.c_int32), ("seg", SqairDenseSeg * 4), ("w", C.c_void_p), ("b", C.c_void_p), ("add", C.c_void_p),
                ("add_ld", C.c_int32), ("add_n", C.c_int32), ("add_rdiv", C.c_int32), ("act_a", C.c_int32), ("act_b", C.c_int32),
                ("act_split", C.c_int32), ("scale", C.c_float), ("scale_ptr", C.c_void_p), ("out", C.c_void_p), ("out_ld", C.c_int32),
                ("M", C.c_int32), ("N", C.c_int32), ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


class SqairDxRange(C.Structure):
    _fields_ = [("n0", C.c_int32), ("n1", C.c_int32), ("dst", C.c_void_p), ("dst_ld", C.c_int32), ("dst2", C.c_void_p),
                ("dst2_ld", C.c_int32), ("add", C.c_void_p), ("add_ld", C.c_int32), ("saved", C.c_void_p), ("saved_ld", C.c_int32),
                ("act_a", C.c_int32), ("act_b", C.c_int32), ("act_split", C.c_int32)]


class SqairDxGru(C.Structure):
    _fields_ = [("mode", C.c_int32), ("g0", C.c_void_p), ("g0_ld", C.c_int32), ("g1", C.c_void_p), ("g1_ld", C.c_int32),
                ("hprev", C.c_void_p), ("h_ld", C.c_int32), ("dpre1", C.c_void_p), ("dp_ld", C.c_int32), ("d_h", C.c_void_p),
                ("dh_ld", C.c_int32), ("acc_dh", C.c_int32), ("dup", C.c_void_p), ("dup_ld", C.c_int32), ("dup_h_off", C.c_int32),
                ("nh", C.c_int32)]


class SqairDxTest(C.Structure):
    """One launch of the routed dX GEMM (include/sqair_hip.h: sqair_linear_dx_test); device addresses, handed on unchanged."""
    _fields_ = [("dpre", C.c_void_p), ("ld", C.c_int32), ("width", C.c_int32), ("M", C.c_int32), ("w", C.c_void_p),
                ("Kdim", C.c_int32), ("scale_ptr", C.c_void_p), ("nranges", C.c_int32), ("r", SqairDxRange * 3), ("gru", SqairDxGru),
                ("scratch", C.c_void_p), ("scratch_bytes", C.c_int64)]


def _fields(spec):
    """'p name' = device address, 'i name' = int32; in the header's order."""
    return [(s.split()[1], C.c_void_p if s.split()[0] == "p" else C.c_int32) for s in spec]


class SqairSlotTailBwdTest(C.Structure):
    """One launch of the slot-tail adjoint (include/sqair_hip.h: sqair_slot_tail_bwd_test); device addresses, handed on unchanged."""
    _fields_ = _fields(["i is_disc", "i slot", "i B", "i enc_pre", "p rec_prev", "p rec_new", "p d_rec_new", "p d_rec_prev", "p s1h",
                        "i s1h_ld", "p hraw", "i h_ld", "p enc", "i enc_ld", "p noise", "p flat", "p d_s1pre", "i ds_ld", "p d_s1pre2",
                        "i ds2_ld", "p d_raw_out", "i dr_ld", "p d_enc", "i de_ld", "p d_hraw", "i dh_ld"])


class SqairCropChainBwdTest(C.Structure):
    """One launch of the crop adjoint of the recurrence (include/sqair_hip.h: sqair_crop_chain_bwd_test)."""
    _fields_ = _fields(["i mode", "i slot", "i B", "i mask_dact", "p img", "p rec_prev", "p rec_new", "p d_rec_prev", "p d_rec_new", "p wb",
                        "i wb_ld", "p d_wb", "p mask", "i mask_row_mul", "i mask_row_add", "p d_mask", "p g_out", "i g_row_mul",
                        "i g_row_add", "p tp", "i tp_ld", "p d_tp", "i dtp_ld", "p noise", "p flat", "p w3", "p t2", "i t2_ld", "p d_t2",
                        "i dt2_ld"])


class SqairWhereParamGradsTest(C.Structure):
    """The batched where-parameter reduction (include/sqair_hip.h: sqair_where_param_grads_test)."""
    _fields_ = _fields(["i T", "i B", "p d_tp", "i tp_ld", "p d_rec_p", "p rec_p", "p noise", "p flat_grad"])


class SqairGruGatesBwdTest(C.Structure):
    """Both stages of the slot RNN's GRU gate adjoints (include/sqair_hip.h: sqair_gru_gates_bwd_test)."""
    _fields_ = _fields(["i rows", "i accumulate_dh", "p d_hn", "i dhn_ld", "p z", "i z_ld", "p r", "i r_ld", "p hc", "i hc_ld", "p hprev",
                        "i h_ld", "p d_rh", "i drh_ld", "p dpre1", "i dp_ld", "p d_h", "i dh_ld", "p dup_z", "i dupz_ld", "i dup_h_off",
                        "p dup_r", "i dupr_ld"])


class SqairLogprobTest(C.Structure):
    """One launch of k_logprob over T frames (include/sqair_hip.h: sqair_logprob_test); device addresses, handed on unchanged."""
    _fields_ = _fields(["i B", "i T", "i t", "i t_global", "p t_row", "p rec_p", "p rec_d", "p rec_prev", "p pstats", "i ps_ld", "p spre",
                        "p flat", "p qz", "p pz", "p disc_lp", "p out"])   # out: the address of a SqairOutputs, or NULL


class SqairLogprobBwdTest(C.Structure):
    """One launch of k_logprob_bwd over T frames (include/sqair_hip.h: sqair_logprob_bwd_test)."""
    _fields_ = _fields(["i B", "i T", "i t_global0", "i ps_ld", "p t_row", "p rec_p", "p rec_d", "p rec_m", "p pstats", "p spre", "p g_lw",
                        "p g_dl", "p d_rec_p", "p d_rec_d", "p d_rec_m", "p d_pstats", "p d_spre", "p flat", "p flat_grad"])


class SqairSlotCropTest(C.Structure):
    """One launch of a crop of the slot loop with its where sample (include/sqair_hip.h: sqair_slot_crop_test)."""
    _fields_ = _fields(["i mode", "i slot", "i B", "i specialised", "p img", "p rec_prev", "p rec_new", "p wb", "i wb_ld", "p tp", "i tp_ld",
                        "p t2", "i t2_ld", "p w3", "p noise", "p flat", "p mask", "i mask_row_mul", "i mask_row_add", "p out",
                        "i out_row_mul", "i out_row_add", "p tp_out", "i tp_out_ld"])


class SqairSlotTailTest(C.Structure):
    """One launch of a slot's tail, alone or inside the next slot's RNN layer (include/sqair_hip.h: sqair_slot_tail_test)."""
    _fields_ = _fields(["i is_disc", "i slot", "i B", "i what_done", "p hraw", "i h_ld", "p enc", "i enc_ld", "p rec_prev", "p rec_new",
                        "p noise", "p s1p", "i s1p_ld", "p s1h_out", "i s1h_ld", "p flat", "p packed", "p hid", "i hid_ld", "p add",
                        "i add_ld", "p out", "i out_ld"])


class SqairLinearWhatTest(C.Structure):
    """One launch of a head layer with the what sample in its epilogue (include/sqair_hip.h: sqair_linear_what_test)."""
    _fields_ = _fields(["i mode", "i slot", "i B", "p x", "i x_ld", "p noise", "p enc", "i enc_ld", "p rec_prev", "p rec_new", "p packed"])


# sqair_debug_dense_routes: the families of the two dense launchers, in the order include/sqair_hip.h documents
DENSE_ROUTES = ("fwd_splitk", "fwd_t2", "fwd_rows", "fwd_mt", "fwd_lds", "fwd_big_2x2", "fwd_big_3x2", "fwd_big_3x3", "fwd_big_4x2",
                "dx_nch1", "dx_nch2", "dx_nch3", "dx_nch4", "dx_nch5", "dx_nch6", "dx_nch7", "dx_nch8", "dx_nch9", "dx_nch12", "dx_nch18",
                "dx_t2", "dx_gru1", "dx_gru2", "fwd_strip")


def dense_routes(library=None):
    """{family: launches of it this process has issued or captured so far} for the two dense launchers."""
    v = (C.c_int64 * len(DENSE_ROUTES))()
    n = (library or lib()).sqair_debug_dense_routes(v, len(DENSE_ROUTES))
    assert n == len(DENSE_ROUTES), "the library counts {} dense routes, this binding names {}".format(n, len(DENSE_ROUTES))
    return dict(zip(DENSE_ROUTES, (int(x) for x in v)))


_PROTOS = {
    "sqair_abi_version": (C.c_int, []),
    "sqair_build_id": (C.c_char_p, []),
    "sqair_build_flags": (C.c_char_p, []),
    "sqair_create": (C.c_int, [C.POINTER(SqairConfig), C.POINTER(C.c_void_p)]),
    "sqair_destroy": (C.c_int, [C.c_void_p]),
    "sqair_last_error": (C.c_char_p, [C.c_void_p]),
    "sqair_param_count": (C.c_int64, [C.c_void_p]),
    "sqair_param_entries": (C.c_int, [C.c_void_p]),
    "sqair_param_entry": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int64)]),
    "sqair_packed_bytes": (C.c_int64, [C.c_void_p]),
    "sqair_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "sqair_noise_width": (C.c_int, [C.c_void_p]),
    "sqair_pack_params": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqair_forward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                C.c_int, C.POINTER(SqairOutputs), C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_train_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "sqair_forward_train": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                      C.c_int, C.POINTER(SqairOutputs), C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_graph_capture": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_int, C.c_int, C.POINTER(SqairOutputs), C.c_void_p, C.c_int64,
                                      C.c_void_p]),
    "sqair_graph_launch": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sqair_graph_nodes": (C.c_int, [C.c_void_p]),
    "sqair_elbo": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_void_p,
                             C.c_void_p]),
    "sqair_st_crop": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "sqair_st_insert_loglik": (C.c_int, [C.c_void_p] * 8 + [C.c_int, C.c_void_p]),
    "sqair_linear_test": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                    C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_gru_test": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                 C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_set_workspace_clearing": (C.c_int, [C.c_void_p, C.c_int]),
    "sqair_clear_workspace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sqair_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "sqair_chain_status": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "sqair_check_scales": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "sqair_check_finite": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_char_p, C.c_void_p, C.c_void_p]),
    "sqair_timeline_available": (C.c_int, []),
    "sqair_timeline_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "sqair_timeline_count": (C.c_int, [C.c_void_p]),
    "sqair_timeline_end": (C.c_int, [C.c_void_p]),
    "sqair_timeline_record": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int)]),
    "sqair_lstm_test": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_lstm_cell_bwd_test": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_void_p]),
    "sqair_compact_test_layout": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32), C.c_int]),
    "sqair_compact_test": (C.c_int, [C.c_void_p] * 13 + [C.POINTER(SqairOutputs), C.c_int, C.c_int, C.c_void_p]),
    "sqair_compact_bwd_test": (C.c_int, [C.c_void_p] * 11 + [C.c_int, C.c_void_p]),
    "sqair_get_config":(C.c_int, [C.c_void_p, C.POINTER(SqairConfig)]),
    "sqair_st_crop_bwd": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_void_p]),
    "sqair_st_insert_loglik_bwd": (C.c_int, [C.c_void_p] * 11 + [C.c_int64, C.c_int, C.c_void_p]),
    "sqair_elbo_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "sqair_backward_scratch_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "sqair_backward_decoder": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqair_backward_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "sqair_backward": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p]),
    "sqair_forward_train_carry": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(SqairCarry), C.POINTER(SqairOutputs),
                                                                C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_backward_carry": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int, C.POINTER(SqairCarry), C.c_void_p, C.c_int64,
                                                          C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sqair_forward_train_carry_masked": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(SqairCarry), C.c_void_p,
                                                                       C.POINTER(SqairOutputs), C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_backward_carry_masked": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int, C.POINTER(SqairCarry), C.c_void_p, C.c_void_p,
                                                                 C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "sqair_set_generation_noise": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sqair_state_bytes": (C.c_int64, [C.c_void_p, C.c_int]),
    "sqair_set_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    "sqair_set_smc": (C.c_int, [C.c_void_p, C.POINTER(SqairSmc), C.c_int]),
    "sqair_smc_resample_test": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(SqairSmc),
                                         C.c_void_p]),
    "sqair_history_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_uint32]),
    "sqair_set_history": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_uint32]),
    "sqair_history_trace": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(SqairTraceOutputs), C.c_void_p]),
    "sqair_trace_lane_scratch_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "sqair_history_trace_lane": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(SqairTraceOutputs), C.c_void_p,
                                           C.POINTER(SqairTraceLane), C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_track_lane_test": (C.c_int, [C.c_void_p] * 6 + [C.c_int] * 3 + [C.POINTER(SqairTraceLane), C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_set_observed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "sqair_set_estimate": (C.c_int, [C.c_void_p, C.POINTER(SqairLaneEstimate), C.c_int, C.c_int]),
    "sqair_lane_estimate_test": (C.c_int, [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_int, C.POINTER(SqairLaneEstimate), C.c_void_p]),
    "sqair_set_layers": (C.c_int, [C.c_void_p, C.POINTER(SqairLaneLayers), C.c_int, C.c_int]),
    "sqair_lane_layers_test": (C.c_int, [C.c_void_p] * 6 + [C.c_float, C.c_int, C.c_int, C.c_int, C.POINTER(SqairLaneLayers), C.c_void_p]),
    "sqair_set_score": (C.c_int, [C.c_void_p, C.POINTER(SqairLaneScore), C.c_int, C.c_int]),
    "sqair_lane_score_test": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(SqairLaneScore), C.c_void_p]),
    "sqair_set_identity": (C.c_int, [C.c_void_p, C.POINTER(SqairLaneIdentity), C.c_int, C.c_int]),
    "sqair_lane_identity_test": (C.c_int, [C.c_void_p] * 6 + [C.c_int, C.c_int, C.POINTER(SqairLaneIdentity), C.c_void_p]),
    "sqair_set_score_ids": (C.c_int, [C.c_void_p, C.c_int]),
    "sqair_set_lane_match": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "sqair_set_idf": (C.c_int, [C.c_void_p, C.POINTER(SqairLaneIdf), C.c_int, C.c_int]),
    "sqair_lane_idf_test": (C.c_int, [C.c_void_p] * 5 + [C.c_int, C.c_int, C.POINTER(SqairLaneScore), C.POINTER(SqairLaneIdf), C.c_void_p]),
    "sqair_lane_idf_solve": (C.c_int, [C.c_void_p, C.POINTER(SqairLaneIdf), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "sqair_lane_traj_score": (C.c_int, [C.c_void_p, C.POINTER(SqairLaneTraj), C.POINTER(SqairTrajTruth), C.POINTER(SqairTrajScore),
                                        C.c_int, C.c_int, C.c_void_p]),
    "sqair_forecast_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "sqair_forecast": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p,
                                 C.POINTER(SqairForecastOutputs), C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_forecast_fan_workspace_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "sqair_forecast_fan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                     C.POINTER(SqairForecastOutputs), C.POINTER(SqairForecastLane), C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_forecast_lane_scratch_bytes": (C.c_int64, [C.c_void_p, C.c_int, C.c_int]),
    "sqair_forecast_lane_test": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 4 + [C.POINTER(SqairForecastLane), C.c_void_p, C.c_int64,
                                                                              C.c_void_p]),
    "sqair_fill_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p]),
    "sqair_capture_begin": (C.c_int, [C.c_void_p, C.c_void_p]),
    "sqair_capture_end": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "sqair_capture_launch": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "sqair_add_l2_grad": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "sqair_rmsprop_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float,
                                     C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p]),
    "sqair_linear_bwd_test": (C.c_int, [C.c_void_p] * 8 + [C.c_int] * 4 + [C.c_void_p, C.c_int64, C.c_void_p]),
    "sqair_linear_contract_test": (C.c_int, [C.c_void_p, C.POINTER(SqairDenseContract), C.c_void_p]),
    "sqair_linear_dx_test": (C.c_int, [C.c_void_p, C.POINTER(SqairDxTest), C.c_void_p]),
    "sqair_slot_tail_bwd_test": (C.c_int, [C.c_void_p, C.POINTER(SqairSlotTailBwdTest), C.c_void_p]),
    "sqair_crop_chain_bwd_test": (C.c_int, [C.c_void_p, C.POINTER(SqairCropChainBwdTest), C.c_void_p]),
    "sqair_where_param_grads_test": (C.c_int, [C.c_void_p, C.POINTER(SqairWhereParamGradsTest), C.c_void_p]),
    "sqair_gru_gates_bwd_test": (C.c_int, [C.c_void_p, C.POINTER(SqairGruGatesBwdTest), C.c_void_p]),
    "sqair_logprob_test": (C.c_int, [C.c_void_p, C.POINTER(SqairLogprobTest), C.c_void_p]),
    "sqair_slot_crop_test": (C.c_int, [C.c_void_p, C.POINTER(SqairSlotCropTest), C.c_void_p]),
    "sqair_slot_tail_test": (C.c_int, [C.c_void_p, C.POINTER(SqairSlotTailTest), C.c_void_p]),
    "sqair_linear_what_test": (C.c_int, [C.c_void_p, C.POINTER(SqairLinearWhatTest), C.c_void_p]),
    "sqair_logprob_bwd_test": (C.c_int, [C.c_void_p, C.POINTER(SqairLogprobBwdTest), C.c_void_p]),
    "sqair_debug_dense_routes": (C.c_int, [C.POINTER(C.c_int64), C.c_int]),
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
}

# what include/sqair_hip.h declares: everything but the measurement helpers -- and the one read-out among them that it documents
EXPORTED_SYMBOLS = [n for n in _PROTOS if not n.startswith("sqair_debug") or n == "sqair_debug_dense_routes"]

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

ABI_VERSION = 2
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
        except (OSError, ImportError):   # a binary-only deployment (no csrc/ -- ModuleNotFoundError --, its .hip files stripped, or no
            # include/ beside the package): nothing to compare with
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
