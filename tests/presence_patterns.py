"""Which slot layouts a test case reaches: a classifier of the ORACLE's presence decisions, and coverage gates on its counts.

Compaction (k_compact / k_compact_bwd) is the identity on the propagated slots unless propagation drops an object that has a
survivor behind it.  A case that is meant to test the permutation has to say that it reaches one: `classify` names the layouts per
(frame, particle row) cell, `count` sums them, `require` fails with the whole table when a minimum is missed.  The inputs are
oracle outputs only (`prop_pres`, `disc_pres`, `_prop_prev_presence`), never anything the HIP path computed.
"""
import numpy as np

PATTERNS = ("drop", "hole", "two_holes", "hole_and_disc", "overflow", "full", "empty", "all_dropped", "hole_before_last")


def _np(x):
    return x.detach().numpy() if hasattr(x, "detach") else np.asarray(x)


def classify(prop_pres, disc_pres, prev_pres):
    """prop_pres, disc_pres, prev_pres: [T, R, N] of 0 / 1 -- the propagation and discovery presences of frame t and the merged
    presence of frame t - 1 (the oracle's `_prop_prev_presence`).  Returns {pattern: bool [T, R]}:

      drop              some slot present at t - 1 is absent after propagation
      hole              a present propagated slot sits behind an absent one: compaction moves a propagated object
      two_holes         some survivor has at least two absent slots ahead of it
      hole_and_disc     a hole, and at least one discovery in the same frame
      overflow          n_prop + n_disc > N: discoveries are truncated
      full / empty      N / 0 objects after the merge
      all_dropped       the row had objects and propagation kept none
      hole_before_last  a hole at t < T - 1: a later frame's gradient flows back through the permutation
    """
    p, d, q = (np.asarray(_np(a), dtype=np.float64) > 0.5 for a in (prop_pres, disc_pres, prev_pres))
    assert p.ndim == 3 and p.shape == d.shape == q.shape, (p.shape, d.shape, q.shape)
    T, R, N = p.shape
    absent_ahead = np.cumsum(~p, -1) - (~p)            # absent propagated slots strictly ahead of slot j
    n_prop, n_disc = p.sum(-1), d.sum(-1)
    hole = (p & (absent_ahead >= 1)).any(-1)
    out = dict(
        drop=(q & ~p).any(-1),
        hole=hole,
        two_holes=(p & (absent_ahead >= 2)).any(-1),
        hole_and_disc=hole & (n_disc >= 1),
        overflow=(n_prop + n_disc) > N,
        full=np.minimum(n_prop + n_disc, N) == N,
        empty=(n_prop + n_disc) == 0,
        all_dropped=q.any(-1) & ~p.any(-1),
        hole_before_last=hole & (np.arange(T)[:, None] < T - 1),
    )
    assert tuple(out) == PATTERNS
    return out


def classify_outputs(outputs, N):
    """`classify` on an oracle output dictionary (Model.outputs of oracle/sqair_oracle.py)."""
    g = lambda k: _np(outputs[k])
    T, R = g("prop_pres").shape[:2]
    return classify(g("prop_pres").reshape(T, R, N), g("disc_pres").reshape(T, R, N), g("_prop_prev_presence").reshape(T, R, -1)[..., :N])


def count(patterns):
    c = {k: int(v.sum()) for k, v in patterns.items()}
    c["cells"] = int(next(iter(patterns.values())).size)
    return c


def table(counts):
    return "presence patterns over {} (frame, row) cells: ".format(counts["cells"]) + " ".join(
        "{}={}".format(k, counts[k]) for k in PATTERNS)


def require(counts, **minimums):
    """Fails, with the whole table, when the case does not reach `pattern >= minimum` for every keyword."""
    unknown = [k for k in minimums if k not in PATTERNS]
    assert not unknown, "unknown pattern(s) {}".format(unknown)
    missed = {k: (counts[k], m) for k, m in minimums.items() if counts[k] < m}
    assert not missed, "the case does not reach the presence patterns it is meant to test: {} (have, need); {}".format(
        missed, table(counts))
    return counts


def moved_ids(obj_id):
    """obj_id [T, R, N] (oracle).  Boolean [T, R, N], true at (t, r, j) for t >= 1 where the object in slot j of frame t sat in
    a DIFFERENT slot of frame t - 1: the places where an id must have followed its object rather than its slot."""
    ids = np.asarray(_np(obj_id), dtype=np.float64)
    T, R, N = ids.shape
    moved = np.zeros(ids.shape, bool)
    for t in range(1, T):
        same = ids[t][:, :, None] == ids[t - 1][:, None, :]          # [R, j at t, j' at t - 1]
        same &= (ids[t] >= 0)[:, :, None]
        moved[t] = (same & ~np.eye(N, dtype=bool)[None]).any(-1)
    return moved
