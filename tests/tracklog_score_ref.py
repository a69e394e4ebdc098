"""The float64 reference of track log scoring (include/sqair_hip.h: sqair_lane_tracklog_score, the track log scoring paragraph),
restated from the header and not from the kernel.  NumPy, plain loops over (lane, view, frame).

The table's fp32 words are read as they are; a view's box is the header's fp32 expression (``motion_ref._fma`` for its fmaf), because
the box is DEFINED as those four words.  Everything computed from words is float64: the IoU is ``score_ref.iou64``, the per-frame
assignment ``score_ref.assign`` (keep + greedy) or ``match_ref.assign`` (keep + optimal), the window's identity assignment
``idf_ref.best_scipy``.  Beside every float64 term of ``sums`` stands its fp32 RESTATEMENT -- ``score_ref.iou32`` for the IoU, and for
err and nees numpy float32 in the header's order with ``_fma`` where the header says fmaf --, summed as the header says (each fp32
value converted to float64 and added).  What the two differ by per term is the measured fp32 error; ``bars`` turns it into the bar
of a sum: four times the worst term's error of the case, times the number of terms of the sum in question."""
import collections

import numpy as np

from tests import idf_ref
from tests import match_ref
from tests import score_ref
from tests.motion_ref import _fma

VIEWS = ("filtered", "smooth", "filtered_filled", "smooth_filled")
COUNTS = ("frames", "frames_invalid", "truth", "tp", "fn", "fp", "idsw", "gap_tp", "gap_fp", "nees_n", "gap_nees_n", "idtp", "idfn",
          "idfp")
SUMS = ("iou_sum", "err_sum", "nees_sum", "gap_err_sum", "gap_nees_sum")
TERMS = dict(iou_sum="tp", err_sum="tp", nees_sum="nees_n", gap_err_sum="gap_tp", gap_nees_sum="gap_nees_n")   # how many terms a sum has
TABLE = ("track_id", "frame_index", "state", "size", "filt", "smooth")
SEEN, GAP = 1, 2
F32 = np.float32

Score = collections.namedtuple("Score", "counts sums sums32 term_err assign ov match match_iou scored iou present")


def view_boxes(table, v):
    """(box [lag, B, C, 4] float32 -- the header's words --, present [lag, B, C] bool) of view v."""
    src = np.asarray(table["smooth" if v & 1 else "filt"], F32)
    size, state = np.asarray(table["size"], F32), np.asarray(table["state"])
    box = np.concatenate([_fma(F32(-0.5), size, src[..., 0]), size], -1)
    present = (state == SEEN) | ((state == GAP) if v >> 1 else np.zeros_like(state, bool))
    return box, present


def scored_frames(table, log_valid, truth_valid):
    """(scored [lag, B] bool, invalid [lag, B] bool): point 2."""
    fi = np.asarray(table["frame_index"])
    lag, B = fi.shape
    L = np.asarray(log_valid).shape[1]
    scored, invalid = np.zeros((lag, B), bool), np.zeros((lag, B), bool)
    for b in range(B):
        for f in range(lag):
            if fi[f, b] < 0 or truth_valid[f, b] == 0:
                continue
            ok = log_valid[b, int(fi[f, b] % L)] != 0
            scored[f, b], invalid[f, b] = ok, not ok
    return scored, invalid


def pair32(t, p_y, p_x, ppy, ppx):
    """Point 4 in numpy float32, the header's operations in the header's order: (err, nees, whether nees counts)."""
    t = np.asarray(t, F32)
    ty, tx = _fma(F32(0.5), t[2], t[0]), _fma(F32(0.5), t[3], t[1])
    dy, dx = F32(ty - F32(p_y)), F32(tx - F32(p_x))
    err = np.sqrt(_fma(dy, dy, F32(dx * dx)))
    honest = bool(ppy > 0 and ppx > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        nees = F32(F32(F32(dy * dy) / F32(ppy)) + F32(F32(dx * dx) / F32(ppx)))
    return F32(err), nees, honest


def pair64(t, p_y, p_x, ppy, ppx):
    """Point 4 in float64 on the same words."""
    t = np.asarray(t, np.float64)
    dy, dx = t[0] + 0.5 * t[2] - float(p_y), t[1] + 0.5 * t[3] - float(p_x)
    honest = bool(ppy > 0 and ppx > 0)
    return float(np.hypot(dy, dx)), (dy * dy / float(ppy) + dx * dx / float(ppx)) if honest else 0.0, honest


def score(table, log_valid, truth, iou_min, match="greedy"):
    """Points 1 to 6.  ``table``: {name: array} of TABLE (track_id [B, C], frame_index [lag, B], state [lag, B, C], size [lag, B, C, 2],
    filt, smooth [lag, B, C, 2, 5] float32); ``log_valid`` [B, L]; ``truth``: dict(truth_box [lag, B, G, 4] float32, truth_present
    [lag, B, G], truth_valid [lag, B]) in window order; ``match``: "greedy" or "optimal"."""
    assign_fn = dict(greedy=score_ref.assign, optimal=match_ref.assign)[match]
    iou_min = float(F32(iou_min))
    tbox, tpres_all, tvalid = (np.asarray(truth[k]) for k in ("truth_box", "truth_present", "truth_valid"))
    lag, B, G = tpres_all.shape
    track_id = np.asarray(table["track_id"])
    C = track_id.shape[1]
    state = np.asarray(table["state"])
    scored, invalid = scored_frames(table, np.asarray(log_valid), tvalid)
    counts = np.zeros((B, 4, len(COUNTS)), np.int64)
    sums, sums32 = np.zeros((B, 4, len(SUMS))), np.zeros((B, 4, len(SUMS)))
    term_err = {n: 0.0 for n in SUMS}
    assign = -np.ones((4, B, G), np.int32)
    ov = np.zeros((B, 4, G, C), np.int64)
    m_out, m_iou = -np.ones((4, lag, B, G), np.int32), np.zeros((4, lag, B, G))
    ious, presents = [], []
    K, S = {n: i for i, n in enumerate(COUNTS)}, {n: i for i, n in enumerate(SUMS)}
    for v in range(4):
        box, cpres_all = view_boxes(table, v)
        src = np.asarray(table["smooth" if v & 1 else "filt"], F32)
        iou = score_ref.iou_table(tbox, box)                                   # [lag, B, G, C] float64
        iou32 = score_ref.iou32(np.asarray(tbox, F32)[:, :, :, None, :], box[:, :, None, :, :]).astype(np.float64)
        ious.append(iou)
        presents.append(cpres_all)
        for b in range(B):
            last = -np.ones(G, np.int64)
            c_ = counts[b, v]
            for f in range(lag):
                if invalid[f, b]:
                    c_[K["frames_invalid"]] += 1
                if not scored[f, b]:
                    continue
                tpres, cpres = tpres_all[f, b] != 0, cpres_all[f, b]
                cand = tpres[:, None] & cpres[None, :]
                with np.errstate(invalid="ignore"):
                    ov[b, v] += cand & (iou[f, b] >= iou_min)
                m, claimed = assign_fn(iou[f, b], tpres, cpres, track_id[b], last, iou_min)
                c_[K["frames"]] += 1
                for g in range(G):
                    if not tpres[g]:
                        continue
                    c_[K["truth"]] += 1
                    c = int(m[g])
                    if c < 0:
                        c_[K["fn"]] += 1
                        continue
                    c_[K["tp"]] += 1
                    c_[K["idsw"]] += int(last[g] >= 0 and last[g] != track_id[b, c])
                    last[g] = track_id[b, c]
                    m_out[v, f, b, g], m_iou[v, f, b, g] = c, iou[f, b, g, c]
                    k = src[f, b, c]
                    args = (tbox[f, b, g], k[0, 0], k[1, 0], k[0, 2], k[1, 2])
                    e64, n64, honest = pair64(*args)
                    e32, n32, honest32 = pair32(*args)
                    assert honest == honest32
                    gap = state[f, b, c] == GAP
                    for name, on, a, r in (("iou_sum", True, iou[f, b, g, c], iou32[f, b, g, c]), ("err_sum", True, e64, e32),
                                           ("nees_sum", honest, n64, n32), ("gap_err_sum", gap, e64, e32),
                                           ("gap_nees_sum", gap and honest, n64, n32)):
                        if on:
                            sums[b, v, S[name]] += float(a)
                            sums32[b, v, S[name]] += float(r)
                            term_err[name] = max(term_err[name], abs(float(r) - float(a)))
                    c_[K["nees_n"]] += int(honest)
                    c_[K["gap_tp"]] += int(gap)
                    c_[K["gap_nees_n"]] += int(gap and honest)
                un = cpres & ~claimed
                c_[K["fp"]] += int(un.sum())
                c_[K["gap_fp"]] += int((un & (state[f, b] == GAP)).sum())
            idtp, r2c = idf_ref.best_scipy(ov[b, v])
            assign[v, b] = r2c
            c_[K["idtp"]], c_[K["idfn"]] = idtp, c_[K["truth"]] - idtp
            c_[K["idfp"]] = c_[K["tp"]] + c_[K["fp"]] - idtp                   # (tp + fp: the present columns over the scored frames)
    return Score(counts, sums, sums32, term_err, assign, ov, m_out, m_iou, scored, ious, presents)


def bars(ref):
    """[B, 4, 5]: the bar of every sum -- four times the case's worst fp32 error of a term of that sum, times its number of terms."""
    K = {n: i for i, n in enumerate(COUNTS)}
    return np.stack([4.0 * ref.term_err[n] * ref.counts[:, :, K[TERMS[n]]] for n in SUMS], -1)


def fragile(ref, truth, iou_min):
    """[(lane, view)] that are fragile by ``score_ref.fragile_from``'s rule applied per view: a candidate IoU within 1e-5 of iou_min,
    or two competing candidates within 1e-5 of each other, on a scored frame."""
    out = []
    for v in range(4):
        lag, B = ref.scored.shape
        first = score_ref.fragile_from(ref.iou[v], ref.present[v], np.where(ref.scored, 0, -1), truth["truth_present"], truth["truth_valid"],
                                       iou_min)
        out += [(b, v) for b in range(B) if first[b] < lag]
    return out


def check_assign(ov, assign, idtp):
    """``assign`` [G] (columns, -1 none) is one-to-one and its overlaps sum to ``idtp``: ``idf_ref.check_assign``'s judgement on columns."""
    cols = [int(c) for c in assign if c >= 0]
    assert len(set(cols)) == len(cols), assign
    assert all(0 <= c < ov.shape[1] for c in cols), assign
    assert all(ov[g, int(c)] > 0 for g, c in enumerate(assign) if c >= 0), assign
    assert sum(int(ov[g, int(c)]) for g, c in enumerate(assign) if c >= 0) == idtp, (assign, idtp)


def pooled(counts, sums, v):
    """The pooled figures of view v over the lanes of counts [B, 4, 14] and sums [B, 4, 5]; NaN where a denominator is 0."""
    c = dict(zip(COUNTS, np.asarray(counts)[:, v].sum(0).tolist()))
    s = dict(zip(SUMS, np.asarray(sums)[:, v].sum(0).tolist()))
    div = lambda a, b: float(a) / b if b else float("nan")
    return dict(mota=1.0 - div(c["fn"] + c["fp"] + c["idsw"], c["truth"]), motp=div(s["iou_sum"], c["tp"]),
                idf1=div(2 * c["idtp"], 2 * c["idtp"] + c["idfp"] + c["idfn"]), idp=div(c["idtp"], c["idtp"] + c["idfp"]),
                idr=div(c["idtp"], c["idtp"] + c["idfn"]), mean_err=div(s["err_sum"], c["tp"]), nees=div(s["nees_sum"], c["nees_n"]),
                gap_err=div(s["gap_err_sum"], c["gap_tp"]), gap_nees=div(s["gap_nees_sum"], c["gap_nees_n"]),
                gap_precision=div(c["gap_tp"], c["gap_tp"] + c["gap_fp"]))
