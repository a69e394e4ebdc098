"""-m gpu: the IDF1 solve alone (k_lane_idf_solve and its device function sq_assign_optimal_i32, through sqair_lane_idf_solve) on
synthetic tables against tests/idf_ref.py, 256 lanes per case, both libraries.  (G, P) = (1, 1), (4, 8), (5, 6) -- also against brute
force --, (16, 64), (16, 4) -- more rows than columns --, (3, 64), (7, 33); lane b has weight regime b % 6: 0..3 (many ties), 0..2^20,
90 % zeros, all zero, a permuted diagonal, free columns in the middle holding stale words.  Everything is integer and compared
exactly: IDTP and all twelve figures equal the reference's; ``assign`` is one-to-one over the used columns and its weight sums to
IDTP -- it is not compared element-wise, because optimal assignments tie.  Also: ``close`` on a subset of the lanes frees those and
only those, totals after two closes are the sum, ``open`` and ``assign`` are optional.  No tolerance is involved.  With
SQAIR_PARITY_DIR set the cases are recorded in idf_parity.json there."""
import functools

import numpy as np
import pytest

from tests import idf_ref as R
from tests.abi_host import LANE_LIBS as LIBS
from tests.idf_cases import record, run_solve, to_device

pytestmark = pytest.mark.gpu

B = 256
SHAPES = [(1, 1), (4, 8), (5, 6), (16, 64), (16, 4), (3, 64), (7, 33)]
REGIMES = ("ties_0_3", "up_to_2^20", "mostly_zero", "all_zero", "permuted_diagonal", "free_columns")


@functools.lru_cache(maxsize=None)
def make_tables(G, P):
    """A table of B lanes {name: array} in the regimes above; made once, never written to."""
    rng = np.random.default_rng(100 * G + P)
    t = R.new_table(B, G, P)
    for b in range(B):
        regime = b % len(REGIMES)
        w = {0: lambda: rng.integers(0, 4, (G, P)), 1: lambda: rng.integers(0, 1 << 20, (G, P)),
             2: lambda: rng.integers(1, 200, (G, P)) * (rng.uniform(size=(G, P)) < 0.1), 3: lambda: np.zeros((G, P), np.int64),
             4: lambda: np.zeros((G, P), np.int64), 5: lambda: rng.integers(0, 50, (G, P))}[regime]()
        if regime == 4:
            n = min(G, P)
            w[rng.permutation(G)[:n], rng.permutation(P)[:n]] = rng.integers(1, 1000, n)
        used = np.ones(P, bool)
        if regime == 5 and P >= 3:
            used[rng.permutation(np.arange(1, P - 1))[:max(1, (P - 2) // 2)]] = False
        elif regime != 4:
            used[int(rng.integers(1, P + 1)):] = False            # the columns taken so far: a prefix, as the kernel fills them
        t["col_id"][b] = np.where(used, rng.permutation(4096)[:P] * 257 + 5, -1)   # (distinct non-negative words)
        t["overlap"][b] = np.where(used[None, :], w, rng.integers(0, 1 << 20, (G, P)))      # stale words in the free columns
        t["col_frames"][b] = np.where(used, w.max(0) + rng.integers(0, 20, P), rng.integers(0, 1 << 20, P))
        t["row_frames"][b] = (w * used[None, :]).max(1) + rng.integers(0, 20, G) * (rng.uniform(size=G) < 0.8)
        t["matched"][b] = (t["row_frames"][b] * rng.choice([0.0, 0.1, 0.2, 0.5, 0.8, 1.0], G)).astype(np.int32)
        t["frag"][b] = rng.integers(0, 4, G)
        t["trk_state"][b] = rng.integers(0, 4, G)
        t["extra_frames"][b] = rng.integers(0, 30)
        t["frames"][b] = 0 if regime == 3 and b % 12 == 3 else int(t["row_frames"][b].max()) + 1
        t["totals"][b] = rng.integers(0, 1 << 40, len(R.TOTALS))
    for a in t.values():
        a.setflags(write=False)
    return t


def same_table(d, t):
    return [n for n in t if not np.array_equal(d[n].cpu().numpy(), t[n])]


@pytest.mark.parametrize("lib_name", list(LIBS))
@pytest.mark.parametrize("G, P", SHAPES, ids=["G{}_P{}".format(*s) for s in SHAPES])
def test_solve_against_the_reference(G, P, lib_name):
    t = make_tables(G, P)
    d = to_device(t)
    open_, assign = run_solve(lib_name, d, G, P)
    ref, ref_open = R.solve(t)
    assert not same_table(d, t)                                   # without close nothing changes
    assert np.array_equal(open_, ref_open), np.argwhere(open_ != ref_open)[:6]
    idtp = R.TOTALS.index("idtp")
    for b in range(B):
        R.check_assign(t, b, assign[b], int(ref_open[b, idtp]))
        if G <= 5 and P <= 6:
            assert R.figures(t, b, R.best_brute)[0][idtp] == open_[b, idtp]
    by_regime = {r: int(ref_open[i::len(REGIMES), idtp].sum()) for i, r in enumerate(REGIMES)}
    print("G{} P{} {}: idtp by regime".format(G, P, lib_name), by_regime)
    record("solve", "G{}_P{}_{}".format(G, P, lib_name), lanes=B, idtp_by_regime=by_regime)
    assert by_regime["all_zero"] == 0 and by_regime["permuted_diagonal"] > 0 and by_regime["ties_0_3"] > 0


@pytest.mark.parametrize("lib_name", list(LIBS))
@pytest.mark.parametrize("G, P", [(4, 8), (16, 64), (16, 4)])
def test_close_frees_those_lanes_only_and_totals_add_up(G, P, lib_name):
    t = make_tables(G, P)
    d = to_device(t)
    close = (np.arange(B) % 3 == 1).astype(np.int32)
    open_, _ = run_solve(lib_name, d, G, P, close=close)
    ref, ref_open = R.solve(t, close=close)
    assert np.array_equal(open_, ref_open) and not same_table(d, ref)
    got = {n: v.cpu().numpy() for n, v in d.items()}
    kept = close == 0
    assert all(np.array_equal(got[n][kept], t[n][kept]) for n in t)
    assert (got["col_id"][~kept] == -1).all() and not got["frames"][~kept].any() and not got["row_frames"][~kept].any()
    assert np.array_equal(got["overlap"], t["overlap"]) and np.array_equal(got["col_frames"], t["col_frames"])   # stale, never read
    assert np.array_equal(got["totals"][~kept], t["totals"][~kept] + ref_open[~kept])
    # a second close of every lane: the freed ones add an empty clip -- nothing --, the others their figures; open / assign optional
    ref2, ref_open2 = R.solve(ref, close=np.ones(B, np.int32))
    assert run_solve(lib_name, d, G, P, close=np.ones(B, np.int32), want_open=False, want_assign=False) == (None, None)
    assert not same_table(d, ref2) and not ref_open2[~kept].any()
    assert np.array_equal(d["totals"].cpu().numpy(), t["totals"] + ref_open)
    for opts in (dict(want_open=False), dict(want_assign=False)):
        e = to_device(t)
        o, a = run_solve(lib_name, e, G, P, close=close, **opts)
        assert not same_table(e, ref) and (o is None or np.array_equal(o, ref_open)) and (a is None or (a >= -1).all())
