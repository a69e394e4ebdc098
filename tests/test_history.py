"""-m gpu: the track history (include/sqair_hip.h: sqair_set_history / sqair_history_trace; SqairStream(history=L).tracks()).

Every case is compared BIT FOR BIT with tests/history_ref.py run on the step() outputs and the source maps recorded on the host:
a hand-driven genealogy on a plain stream, SMC with caller uniforms and adaptive SMC, chunks / a wrapping ring / lag < L / the wide
library / the slot chain / K = 1, the stream left unchanged by the history, graph replay and node counts, the track table, and
the weights against forecast()'s."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.stream import SqairStream
from tests import history_ref as H
from tests.stream_harness import FIELD_OF, OUTS, core, history_check, history_push, host, setup

pytestmark = pytest.mark.gpu

HW = (50, 50)


def _setup(flags, B, T, seed=11):
    return setup(flags, B, T, HW, seed)


def _core(F, P, options=None):
    return core(F, HW, P, options)


# ---- (a) a hand-driven genealogy on a plain stream ---------------------------------------------------------------------------
def test_deterministic_genealogy():
    B, K, T, L = 2, 4, 12, 8
    F, P, obs, noise = _setup(dict(k_particles=K, n_steps_per_image=3), B, T)
    st = SqairStream(_core(F, P), B, outputs=OUTS, history=L)
    R = B * K
    script = {2: ("resample", [0, 0, 2, 3, 4, 5, 5, 5]), 3: ("resample", [1, 1, 1, 2, 7, 6, 5, 4]), 5: ("reset", [1]),
              6: ("resample", [3, 3, 3, 3, 4, -1, 6, 6]), 8: ("resample", [0, 1, 2, 3, 5, 5, 7, 7]), 9: ("resample", [2, 2, 0, 0, 4, 5, 6, 7]),
              10: ("reset", [0])}
    rec = H.Recorder(R)
    history_check(st, rec, "next", st.carried.pending())      # nothing pushed yet: every frame invalid
    coalesced = moved = False
    for t in range(T):
        if t in script:
            getattr(st, script[t][0])(script[t][1])
        parent = st.carried.pending().copy()
        history_push(rec, parent, host(st.step(obs[t:t + 1], noise=noise[t:t + 1])))
        last = history_check(st, rec, "last")
        history_check(st, rec, "last", lag=3)
        if t + 1 in script:                            # the map armed for the next step is where "next" starts from
            getattr(st, script[t + 1][0])(script[t + 1][1])
            script.pop(t + 1)
        nxt = history_check(st, rec, "next", st.carried.pending())
        for o in (last, nxt):
            ua, anc = o["unique_ancestors"], o["ancestor_row"]
            coalesced |= bool(((ua < K) & (ua > 0)).any())
            moved |= bool(((anc >= 0) & (anc != np.arange(R)[None, :])).any())
    # the precondition of this test: it cannot pass on identity maps alone
    assert coalesced and moved
    assert len(rec.steps) > L       # ... and the ring has wrapped


# ---- (b) SMC at every step, caller uniforms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5, 16])
def test_smc_every_step(K):
    B, T, L = 3, 9, 6
    F, P, obs, noise = _setup(dict(k_particles=K, n_steps_per_image=3), B, T, seed=3)
    st = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=1.0, history=L)
    rec = H.Recorder(B * K)
    rng = np.random.default_rng(5)
    parent = np.full(B * K, -1)
    history_check(st, rec, "next", parent)
    moved = False
    for t in range(T):
        o = host(st.step(obs[t:t + 1], noise=noise[t:t + 1], uniforms=rng.uniform(size=B).astype(np.float32)))
        history_push(rec, parent, o)
        parent = o["ancestors"]
        moved |= not np.array_equal(parent, np.arange(B * K))
        history_check(st, rec, "last")
        got = history_check(st, rec, "next", parent)
        assert np.allclose(got["weights"], 1.0 / K, rtol=1e-6, atol=0)   # resampled: the surviving set is equally weighted
        assert np.array_equal(got["best_row"], np.arange(B) * K)
    assert moved and (got["unique_ancestors"][0] <= got["unique_ancestors"][-1]).all()


# ---- (c) adaptive SMC over a longer stream; the maps are the returned ancestors ----------------------------------------------
def test_adaptive_smc():
    B, K, T, L = 4, 5, 40, 16
    F, P, obs, _ = _setup(dict(k_particles=K, n_steps_per_image=3), B, T, seed=41)
    st = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=0.5, seed=9, history=L)
    rec = H.Recorder(B * K)
    parent = np.full(B * K, -1)
    went = 0
    for t in range(T):
        o = host(st.step(obs[t:t + 1]))
        history_push(rec, parent, o)
        parent = o["ancestors"]
        went += int(o["resampled"].sum())
        if t % 7 == 6 or t == T - 1:
            history_check(st, rec, "last", lag=5)
            got = history_check(st, rec, "next", parent)
            first = np.array([int(np.flatnonzero(row == row.max())[0]) for row in got["weights"]])
            assert np.array_equal(got["best_row"], np.arange(B) * K + first)
    assert 0 < went < B * T
    assert (got["unique_ancestors"][0] < K).any() and (got["frame_index"][-1] == T - 1).all()


# ---- (d) shapes and options ---------------------------------------------------------------------------------------------------
CASES = {
    "chunks_T5": (dict(k_particles=3, n_steps_per_image=3), dict(frames_per_step=5), None),
    "wide_n_what64": (dict(k_particles=3, n_steps_per_image=3, n_what=64), dict(), None),
    "slot_chain": (dict(k_particles=3, n_steps_per_image=3), dict(), {"slot_chain": 1}),
    "K1": (dict(k_particles=1, n_steps_per_image=3), dict(), None),
    "mandatory_fields": (dict(k_particles=3, n_steps_per_image=3), dict(history_fields=()), None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_shapes_and_options(case):
    flags, kw, options = CASES[case]
    Tp = kw.get("frames_per_step", 1)
    B, steps, L = 2, 5, 3                                   # L smaller than the stream: the ring wraps
    F, P, obs, noise = _setup(flags, B, steps * Tp, seed=7)
    K = int(F.k_particles)
    core = _core(F, P, options=options)
    if "n_what" in flags:
        assert core.lib is _capi.lib(_capi.WIDE_LIB_PATH)
    smc = K > 1
    st = SqairStream(core, B, outputs=OUTS, history=L, **(dict(resample="systematic", ess_frac=1.0, seed=5) if smc else {}), **kw)
    fields = tuple(k for k, v in FIELD_OF.items() if v in st.history_fields)
    assert fields == (tuple(FIELD_OF) if "history_fields" not in kw else ("where", "presence", "obj_id"))
    rec = H.Recorder(B * K)
    parent = np.full(B * K, -1)
    for s in range(steps):
        if not smc and s == 3:
            st.reset([1])
        if not smc:
            parent = st.carried.pending().copy()
        o = host(st.step(obs[s * Tp:(s + 1) * Tp], noise=noise[s * Tp:(s + 1) * Tp]))
        history_push(rec, parent, o, fields)
        nxt = o["ancestors"] if smc else st.carried.pending()
        for lag in (1, 2, L):                               # lag < L and lag = L
            history_check(st, rec, "last", lag=lag, fields=fields)
            got = history_check(st, rec, "next", nxt, lag=lag, fields=fields, table=(lag == L))
            assert got["where"].shape == (lag * Tp, B * K, 3, 4)
        parent = nxt
    assert ("what" in got) == ("what" in fields) and ("log_w" in got) == ("log_w" in fields)
    if options:
        core.check_chain()
    if not smc:
        assert (got["frame_index"][-1] == [steps * Tp - 1, 1 * Tp + Tp - 1]).all()      # lane 1 restarted at step 3


# ---- (e) history on leaves the stream unchanged -------------------------------------------------------------------------------
@pytest.mark.parametrize("smc", [False, True])
def test_history_leaves_the_stream_unchanged(smc):
    B, T = 3, 8
    F, P, obs, noise = _setup(dict(k_particles=4, n_steps_per_image=3), B, T, seed=23)
    kw = dict(resample="systematic", ess_frac=0.5, seed=3) if smc else {}
    a = SqairStream(_core(F, P), B, outputs=OUTS, **kw)
    b = SqairStream(_core(F, P), B, outputs=OUTS, history=4, **kw)
    for t in range(T):
        b.tracks(start="next" if t % 2 else "last", lag=1 + t % 4)
        if not smc and t == 4:
            a.resample(np.arange(B * 4)[::-1].copy())
            b.resample(np.arange(B * 4)[::-1].copy())
        oa, ob = host(a.step(obs[t:t + 1], noise=noise[t:t + 1])), host(b.step(obs[t:t + 1], noise=noise[t:t + 1]))
        assert set(oa) == set(ob)
        for k in oa:
            assert H.same_bits(oa[k], ob[k]), (k, t)
        names = ("state", "log_weight_sum") + (("log_z", "log_evidence", "ess", "u", "resampled", "_src") if smc else ())
        for n in names:
            assert H.same_bits(getattr(a, n).cpu().numpy(), getattr(b, n).cpu().numpy()), (n, t)
    assert a.history is None and b.history == 4
    with pytest.raises(ValueError, match="keeps no history"):
        a.tracks()
    for bad in (dict(lag=0), dict(lag=5), dict(lag=1.5), dict(start="first"), dict(max_tracks=0), dict(max_tracks=1025)):
        with pytest.raises(ValueError, match=r"^SqairStream\.tracks: "):
            b.tracks(**bad)


# ---- (f) graph replay equals eager; one node more --------------------------------------------------------------------------------
def test_graph_replay_equals_eager():
    B, K, T, L = 4, 4, 12, 5
    F, P, obs, _ = _setup(dict(k_particles=K, n_steps_per_image=3), B, T, seed=29)
    runs = []
    for use_graph in (False, True):
        st = SqairStream(_core(F, P), B, outputs=OUTS, use_graph=use_graph, seed=3, resample="systematic", ess_frac=0.5, history=L)
        rec, parent, out = H.Recorder(B * K), np.full(B * K, -1), []
        for t in range(T):
            o = host(st.step(obs[t:t + 1]))
            history_push(rec, parent, o)
            parent = o["ancestors"]
            out.append((o, history_check(st, rec, "next", parent), history_check(st, rec, "last", lag=2)))
        runs.append(out)
        st.close()      # history and state off: the trace is refused again
        o = _capi.SqairTraceOutputs(T=1)
        assert st.core.lib.sqair_history_trace(st.core.handle, st.carried.ring.data_ptr(), None, 1, C.byref(o), None) == -1
    for (oe, ne, le), (og, ng, lg) in zip(*runs):
        for e, g in ((oe, og), (ne, ng), (le, lg)):
            assert set(e) == set(g)
            for k in e:
                assert H.same_bits(e[k], g[k]), k


def test_graph_has_exactly_one_node_more():
    B = 4
    F, P, obs, noise = _setup(dict(k_particles=2, n_steps_per_image=3), B, 1, seed=51)

    def nodes(**kw):
        core = _core(F, P)
        st = SqairStream(core, B, outputs=OUTS, **kw)
        st.step(obs, noise=noise)
        torch.cuda.synchronize()
        return core.graph_nodes()

    smc = dict(resample="systematic", ess_frac=0.5)
    n_state = nodes()
    assert n_state > 50
    assert nodes(history=None) == n_state and nodes(**smc) == n_state + 1              # off: unchanged
    assert nodes(history=4) == n_state + 1 and nodes(history=64, history_fields=()) == n_state + 1
    assert nodes(history=4, **smc) == n_state + 2


# ---- (g) the track table, a row with more ids than max_tracks included ---------------------------------------------------------
def test_track_table():
    B, K, T, L = 4, 5, 16, 16
    F, P, obs, _ = _setup(dict(k_particles=K, n_steps_per_image=3), B, T, seed=41)
    st = SqairStream(_core(F, P), B, outputs=OUTS, resample="systematic", ess_frac=0.5, seed=9, history=L)
    rec, parent = H.Recorder(B * K), np.full(B * K, -1)
    for t in range(T):
        o = host(st.step(obs[t:t + 1]))
        history_push(rec, parent, o)
        parent = o["ancestors"]
    full = history_check(st, rec, "next", parent)                      # the default M = 2 N
    assert full["track_id"].shape == (B * K, 6)
    n = full["n_tracks"]
    print("n_tracks per row:", n.tolist())
    assert n.max() >= 2, "the stream shows no row with two object ids: the truncation below would not be exercised"
    for M in (1, int(n.max()) - 1, int(n.max()), 9):
        if M < 1:
            continue
        got = history_check(st, rec, "next", parent, max_tracks=M)
        history_check(st, rec, "last", max_tracks=M, lag=7)
        assert np.array_equal(got["n_tracks"], n)               # the true count, whatever M
        assert ((got["track_id"] >= 0).sum(1) == np.minimum(n, M)).all()
    assert (n > 1).any()                                        # M = 1 truncated at least one row
    # a track is present exactly where its id is present in a slot
    pres = (full["presence"] == 1)
    for r in range(B * K):
        for m in range(min(int(n[r]), 6)):
            want = (pres[:, r] & (full["obj_id"][:, r] == full["track_id"][r, m])).any(-1)
            assert np.array_equal(full["track_present"][:, r, m] == 1, want)


# ---- (h) the weights are forecast()'s --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("smc", [False, True])
def test_weights_equal_the_forecasts(smc):
    B, K, T = 3, 4, 6
    F, P, obs, noise = _setup(dict(k_particles=K, n_steps_per_image=3), B, T, seed=13)
    kw = dict(resample="systematic", ess_frac=0.5, seed=3) if smc else {}
    st = SqairStream(_core(F, P), B, outputs=OUTS, history=3, **kw)
    for t in range(T):
        st.step(obs[t:t + 1], noise=noise[t:t + 1])
        if not smc and t == 2:
            st.resample(np.array([1, 1, 2, 3, 4, 4, 4, 7, -1, 9, 10, 11]))
        if t == 4:
            st.reset([0])
        w_t = host(st.tracks(start="next", table=False))
        w_f = host(st.forecast(1, outputs=("presence",)))["weights"]
        assert w_t["weights"].shape == (B, K) and H.same_bits(w_t["weights"], w_f), t
        first = np.array([int(np.flatnonzero(row == row.max())[0]) for row in w_f])
        assert np.array_equal(w_t["best_row"], np.arange(B) * K + first)
