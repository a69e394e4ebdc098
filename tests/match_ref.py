"""The float64 reference of keep + optimal per-frame matching (include/sqair_hip.h: sqair_set_lane_match), restated from the header
and not from the kernel.  Keep is tests/score_ref.py's; the rest is the optimum of the header's integer table -- 2^25 + q for an
eligible pair of an unmatched row and an unclaimed column, q = the IoU in units of 2^-20 rounded to nearest even -- by SciPy's
``linear_sum_assignment``, which tests/test_match_ref.py holds to brute force over all partial assignments (``solve_brute``).

The three references the modes plug into stay as they are (tests/score_ref.py, identity_ref.py, traj_score_ref.py): each calls its
assignment through a module-level name, and ``replaced`` swaps that name for the optimal one -- or for a ``Judge``, which IMPOSES
the device's own matching after judging it: equally optimal assignments tie and the header states no rule among them, so the
events and the memory are compared with a reference run on the device's pairs, and the pairs themselves are held to feasibility,
the optimal cardinality and the optimal sum of q within the rounding of q."""
import contextlib
import json
import os

import numpy as np
from scipy.optimize import linear_sum_assignment

from tests import identity_ref as I
from tests import score_ref as R
from tests import traj_score_ref as TR

UNIT = 1048576.0        # q counts 2^-20
BIG = 1 << 25           # one pair more outweighs every sum of q: at most 16 pairs of q <= 2^20
NEAR = 1e-5
PARITY_DIR_ENV = "SQAIR_PARITY_DIR"


def q_of(iou):
    """q of an IoU (array) in float64 arithmetic: round to nearest, ties to even, as __float2int_rn."""
    return np.rint(np.asarray(iou, np.float64) * UNIT).astype(np.int64)


def keep_step(ok, ids, last):
    """The score's point 2 on the eligibility table ok [G, N]: match [G] (j or -1), claimed [N]."""
    G, N = ok.shape
    match = -np.ones(G, np.int64)
    claimed = np.zeros(N, bool)
    for g in range(G):
        if last[g] < 0:
            continue
        for j in range(N):
            if not claimed[j] and ids[j] == last[g] and ok[g, j]:
                match[g], claimed[j] = j, True
                break
    return match, claimed


def weights(iou, ok, match, claimed):
    """The header's int table [G, N]: BIG + q for an eligible pair of an unmatched row and an unclaimed column, -1 elsewhere."""
    free = ok & (match < 0)[:, None] & ~claimed[None, :]
    with np.errstate(invalid="ignore"):
        return np.where(free, BIG + q_of(np.where(free, iou, 0.0)), -1)


def solve(w):
    """The maximum over all partial one-to-one assignments of the sum of the weights, pairs of negative weight never taken:
    (value, [(g, j), ...]).  A pair of weight 0 in a full assignment of the clipped table is a pair left out."""
    if w.size == 0:
        return 0, []
    rows, cols = linear_sum_assignment(np.maximum(w, 0), maximize=True)
    pairs = [(int(g), int(j)) for g, j in zip(rows, cols) if w[g, j] > 0]
    return int(sum(w[g, j] for g, j in pairs)), pairs


def solve_brute(w):
    """The same maximum by trying every partial assignment (row by row: leave it out, or any free column of non-negative weight)."""
    G, N = w.shape

    def best(g, used):
        if g == G:
            return 0
        top = best(g + 1, used)
        for j in range(N):
            if not used >> j & 1 and w[g, j] >= 0:
                top = max(top, int(w[g, j]) + best(g + 1, used | 1 << j))
        return top
    return best(0, 0)


def keep_optimal(iou, ok, ids, last):
    """Keep, then the optimum of the rest: match [G], claimed [N]."""
    match, claimed = keep_step(ok, ids, last)
    for g, j in solve(weights(iou, ok, match, claimed))[1]:
        match[g], claimed[j] = j, True
    return match, claimed


def _ok(iou, rpres, cpres, iou_min):
    with np.errstate(invalid="ignore"):
        return np.asarray(rpres, bool)[:, None] & np.asarray(cpres, bool)[None, :] & (iou >= iou_min)   # (a NaN fails)


def assign(iou, tpres, lpres, ids, last, iou_min):
    """tests/score_ref.py's ``assign`` in the optimal mode (the same arguments, the same results)."""
    return keep_optimal(iou, _ok(iou, tpres, lpres, iou_min), ids, last)


def link(iou, live, pres, words, keep, iou_min):
    """tests/identity_ref.py's ``_link`` in the optimal mode."""
    return keep_optimal(iou, _ok(iou, live, pres, iou_min), words, keep)[0]


@contextlib.contextmanager
def replaced(module, name, fn):
    """``module.name`` is ``fn`` inside the block: how a reference is run in another mode, or on an imposed matching."""
    old = getattr(module, name)
    setattr(module, name, fn)
    try:
        yield
    finally:
        setattr(module, name, old)


def score(iou_min, **x):
    """tests/score_ref.py's ``score`` with keep + optimal for its points 2 and 3."""
    with replaced(R, "assign", assign):
        return R.score(iou_min=iou_min, **x)


def identity(*a, **k):
    """tests/identity_ref.py's ``identity`` with keep + optimal for its point 2."""
    with replaced(I, "_link", link):
        return I.identity(*a, **k)


def traj_score(tab, tr, iou_min, keep_id=None, **k):
    """tests/traj_score_ref.py's ``score`` with keep + optimal for its point 1."""
    with replaced(TR, "assign", assign):
        return TR.score(tab, tr, iou_min, keep_id, **k)


class Judge(object):
    """Stands for a reference's assignment function and imposes matchings given from outside, judging each on the way.  ``given``:
    an iterable of (key, match [rows] of j or -1) in the order the reference asks; ``skip``: keys that are imposed but not judged (a
    lane past its first fragile frame).  After the run: ``asked`` (how many), ``judged``, and the failures by kind --
    ``infeasible`` (not one-to-one, an ineligible pair, or a kept pair given up), ``cardinality`` (pairs != the optimum's),
    ``deficit`` (the optimum's sum of q minus the given pairs', evaluated here in float64, where it exceeds ``slack(rows, cols)``);
    ``worst_deficit`` over the judged.  An infeasible matching is replaced by the reference's own, so that the run goes on."""

    def __init__(self, given, slack, skip=()):
        self.given, self.slack, self.skip = iter(given), slack, set(skip)
        self.asked = self.judged = 0
        self.infeasible, self.cardinality, self.deficit = [], [], []
        self.worst_deficit = 0

    def _judge(self, key, iou, ok, ids, last, m):
        G, N = ok.shape
        kept, claimed = keep_step(ok, ids, last)
        pairs = [(g, int(m[g])) for g in range(G) if m[g] >= 0]
        cols = [j for _, j in pairs]
        if (len(set(cols)) != len(cols) or any(not 0 <= j < N or not ok[g, j] for g, j in pairs) or
                any(kept[g] >= 0 and m[g] != kept[g] for g in range(G))):
            self.infeasible.append(key)
            return False
        if key in self.skip:
            return True
        self.judged += 1
        w = weights(iou, ok, kept, claimed)
        value, best = solve(w)
        rest = [(g, j) for g, j in pairs if kept[g] < 0]
        if len(rest) != len(best):
            self.cardinality.append((key, len(rest), len(best)))
            return True
        short = value - int(sum(w[g, j] for g, j in rest))
        self.worst_deficit = max(self.worst_deficit, short)
        if short > self.slack(G, N):
            self.deficit.append((key, short))
        return True

    def _next(self, iou, ok, ids, last):
        key, m = next(self.given)
        self.asked += 1
        m = np.array(m, np.int64)
        if not self._judge(key, iou, ok, ids, last, m):
            return keep_optimal(iou, ok, ids, last)
        claimed = np.zeros(ok.shape[1], bool)
        claimed[m[m >= 0]] = True
        return m, claimed

    def assign(self, iou, tpres, lpres, ids, last, iou_min):      # (score_ref.assign, traj_score_ref.assign)
        return self._next(iou, _ok(iou, tpres, lpres, iou_min), ids, last)

    def link(self, iou, live, pres, words, keep, iou_min):        # (identity_ref._link)
        return self._next(iou, _ok(iou, live, pres, iou_min), words, keep)[0]

    def clean(self):
        return not (self.infeasible or self.cardinality or self.deficit)


def slack(e):
    """What the sum of q of an optimal device matching may fall short of the float64 optimum: per pair q moves by at most rounding
    (1/2 each side) plus the fp32 IoU's error e (in units of 2^-20), on the device's pairs and on the optimum's."""
    return lambda rows, cols: 2.0 * min(rows, cols) * (1.0 + e)


def scored_frames(x):
    """The (t, b) tests/score_ref.py's ``score`` asks an assignment for, in its order (lanes outside, frames inside)."""
    T, B = np.asarray(x["truth_valid"]).shape
    return [(t, b) for b in range(B) for t in range(T) if x["truth_valid"][t, b] != 0 and x["map_count"][t, b] != -1]


def fragile_from(iou, rpres, cpres, on, iou_min):
    """[B]: each lane's first frame with a candidate IoU within 1e-5 of iou_min (T where none is).  iou [T, B, G, N], rpres [T, B, G],
    cpres [T, B, N], on [T, B] (the frames that are scored).  No lane is left out for a tie: ties need no rule here."""
    T, B = on.shape
    cand = (np.asarray(rpres) != 0)[..., :, None] & (np.asarray(cpres) != 0)[..., None, :] & np.asarray(on, bool)[..., None, None]
    with np.errstate(invalid="ignore"):
        near = (cand & (np.abs(iou - float(np.float32(iou_min))) <= NEAR)).any((2, 3))
    return np.where(near.any(0), near.argmax(0), T).astype(np.int64)


class IdentityFollower(object):
    """tests/identity_ref.py's ``identity`` carried frame by frame on the DEVICE's own position links: before each frame the
    reference's table says which entry holds which track id, so the device's outputs of the frame -- slot j kept or bridged onto
    ``lane_id`` -- name the entry every linked slot took; that matching is judged (``Judge``) and imposed.  ``kw``: the scalars of
    ``identity`` (iou_min, reid_dist, reid_what, M, max_age, appearance); ``e``: the fp32 IoU's error in units of 2^-20; ``tol``: the
    band of identity_ref's own fragile rule, used when re-identification is on (its compares leave a lane out too).  A lane is left
    out from its first frame with a candidate IoU within 1e-5 of iou_min: ``first`` [B], in frames fed so far (``frames`` where none)."""

    def __init__(self, B, N, nw, kw, e, tol=None):
        self.kw, self.e, self.tol, self.N = kw, e, tol, N
        self.mem = I.fresh_memory(B, kw["M"], nw, kw.get("appearance", True))
        self.first = np.full(B, -1, np.int64)          # -1: not fragile so far
        self.frames = self.asked = self.judged = self.worst = 0
        self.failures = []

    def feed(self, y, how, lane_id):
        """The frames ``y`` (box, presence, obj_id, what, best_row [T', B, ...]) with the device's ``how`` and ``lane_id`` [T', B, N];
        returns the reference's lane_id, how, track_len [T', B, N] on the device's links."""
        kw, M_ = self.kw, self.kw["M"]
        T, B = np.asarray(y["best_row"]).shape
        out = {n: -np.ones((T, B, self.N), np.int32) for n in ("lane_id", "how", "track_len")}
        for t in range(T):
            lanes = [b for b in range(B) if y["best_row"][t, b] != -1]
            iou, _, _ = I.tables(self.mem["trk_box"], y["box"][t], None, None)
            live, pres = self.mem["trk_id"] >= 0, np.asarray(y["presence"][t]) != 0
            with np.errstate(invalid="ignore"):
                near = ((live[:, :, None] & pres[:, None, :]) & (np.abs(iou - float(np.float32(kw["iou_min"]))) <= NEAR)).any((1, 2))
            for b in lanes:
                if near[b] and self.first[b] < 0:
                    self.first[b] = self.frames
            given = []
            for b in lanes:
                m = -np.ones(M_, np.int64)
                for j in range(self.N):
                    if how[t, b, j] in (I.KEPT, I.BRIDGED):
                        e = np.flatnonzero(live[b] & (self.mem["trk_id"][b] == lane_id[t, b, j]))
                        if len(e) == 1:
                            m[e[0]] = j
                given.append((b, m))
            judge = Judge(given, slack(self.e), [b for b in lanes if self.first[b] >= 0])
            with replaced(I, "_link", judge.link):
                step = I.identity(**{k: np.asarray(v)[t:t + 1] for k, v in y.items()}, mem=self.mem, tol=self.tol, **kw)
            if self.tol is not None:
                for b in lanes:
                    if step.fragile_from[b] == 0 and self.first[b] < 0:
                        self.first[b] = self.frames
            self.mem = step.mem
            for n in out:
                out[n][t] = getattr(step, n)[0]
            self.asked, self.judged, self.worst = self.asked + judge.asked, self.judged + judge.judged, max(self.worst, judge.worst_deficit)
            self.failures += [("infeasible", self.frames, b) for b in judge.infeasible if self.first[b] < 0]
            self.failures += [("cardinality", self.frames) + k for k in judge.cardinality] + [("sum of q", self.frames) + k for k in judge.deficit]
            self.frames += 1
        return out

    def whole(self):
        """[B]: lanes compared to the end."""
        return self.first < 0

    def upto(self):
        """[frames, B]: the frames before each lane's first fragile one."""
        return np.arange(self.frames)[:, None] < np.where(self.first < 0, self.frames, self.first)[None, :]


def record(section, case, **figures):
    """Adds ``figures`` to match_parity.json under SQAIR_PARITY_DIR (nothing without it)."""
    where = os.environ.get(PARITY_DIR_ENV)
    if not where:
        return
    path = os.path.join(where, "match_parity.json")
    try:
        os.makedirs(where, exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {}).setdefault(case, {}).update(figures)
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass
