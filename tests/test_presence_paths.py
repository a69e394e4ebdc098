"""-m gpu: the whole path in the regime where objects vanish.

At the initialisation's `prop_step_bias = 5` (and `prop_prior_step_bias = 10`) a propagated object survives with p ~ 0.993, so in
the other suites the slot compaction is almost always the identity on the propagated slots.  Here the same helpers and the same
bars run with `prop_step_bias = 0.0` (`prop_prior_step_bias = 0.0` for forecasts): an initialisation flag, nothing in the product
changes.  Every case first REQUIRES, from the oracle's outputs alone (tests/presence_patterns.py), that it reaches the layouts it
is meant to test -- survivors behind a dropped slot ("holes"), holes with discoveries in the same frame, truncated discoveries,
rows that lose every object, and a hole before the last frame (so that a later frame's gradient flows back through the
permutation) -- and only then compares.  The noise draw is chosen by `stable_noise` on the oracle's margin alone.

Measured margins of these cases: profiles/presence_paths_parity.json.  The kernels on their own: tests/test_compact_kernel.py."""
import json
import os

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.flags import make_flags
from sqair_amd.model import SqairCore
from sqair_amd.stream import SqairStream
from tests import presence_patterns as PP
from tests.hip_util import run_hip, run_oracle
from tests.pass_cases import check_report, full_backward_case, live_oracle_case, live_oracle_inputs, spec_launches
from tests.stream_cases import chunk_two_case, rollout_case
from tests.stream_harness import OUTS, chunked, compare, history_check, history_push, host, one_pass, switches

pytestmark = pytest.mark.gpu

VANISH = dict(prop_step_bias=0.0)
LSTM3 = dict(transition="LSTM", time_transition="LSTM", prior_transition="LSTM")
MINIMUMS = dict(hole=3, hole_and_disc=2, overflow=1, all_dropped=1, hole_before_last=1)
ONE_SLOT = dict(all_dropped=3, overflow=1)    # N = 1: object dropped, row empty, rediscovered

# name: (K, N, T, B, frame, flags, minimums)
FORWARD = {
    "K7N3T4B5": (7, 3, 4, 5, (32, 40), {}, MINIMUMS),
    "K5N4T4B2_shipped_shape": (5, 4, 4, 2, (50, 50), {}, MINIMUMS),
    "K3N3T3B3": (3, 3, 3, 3, (32, 40), {}, MINIMUMS),
    "K3N3T3B3_lstm": (3, 3, 3, 3, (32, 40), LSTM3, MINIMUMS),
    "K3N3T3B3_wide_n_what_64": (3, 3, 3, 3, (32, 40), dict(n_what=64), MINIMUMS),
    "K2N8T3B2": (2, 8, 3, 2, (50, 50), {}, MINIMUMS),
    "K5N1T4B3_one_slot": (5, 1, 4, 3, (32, 40), {}, ONE_SLOT),
}


# cases in which elbo_iwae is judged at 4 x the fp32 oracle's own distance from the fp64 oracle, measured by the test (see there)
FP32_ELBO_IWAE = ("K3N3T3B3_wide_n_what_64",)
PARITY_DIR_ENV = "SQAIR_PARITY_DIR"   # a directory: the cases append their measured figures to presence_paths_parity.json in it


def _record(section, case, **figures):
    """With SQAIR_PARITY_DIR set, appends the case's measured figures to presence_paths_parity.json there (the copy under
    profiles/ is such a file); without it nothing is written."""
    where = os.environ.get(PARITY_DIR_ENV)
    if not where:
        return
    path = os.path.join(where, "presence_paths_parity.json")
    try:
        os.makedirs(where, exist_ok=True)
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {})[case] = dict(build_id=_capi.build_id(), **figures)
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def _forward_inputs(case):
    K, N, T, B, hw, flags, minimums = FORWARD[case]
    F = make_flags(k_particles=K, n_steps_per_image=N, **dict(VANISH, **flags))
    x = live_oracle_inputs(F, hw, T, B)          # (prints the pattern table)
    PP.require(x["counts"], **minimums)
    return F, hw, T, B, N, x


@pytest.mark.parametrize("case", sorted(FORWARD))
def test_forward_where_objects_vanish(case):
    """Every output against the fp64 oracle at `live_oracle_case`'s bar; presence, ids and step counts exact.  Where the oracle
    says an object changed its slot between two frames, the HIP ids must have followed the object.

    K3N3T3B3_wide_n_what_64: elbo_iwae = 0.5433 is a log-mean-exp of log weights up to 660 in size, so the helper's bar (1e-4
    absolute for |ref| < 1) is 1.5e-7 of its operands; the case is judged at 4 x the fp32 oracle's own distance from the fp64
    oracle, measured here on the same inputs.  It is the case that exposed the coherent rounding of the likelihood's per-pixel
    constant in k_insert_loglik: before that fix HIP was 2.93e-4 from the fp64 oracle against 6.38e-5 for the fp32
    oracle (4.6 x); figures after it in profiles/presence_paths_parity.json."""
    F, hw, T, B, N, x = _forward_inputs(case)
    bars = None
    if case in FP32_ELBO_IWAE:
        # The case exceeds the helper's bar on elbo_iwae.  Whether that is rounding is measured, not assumed: the fp32 ORACLE on the
        # same inputs, its distance from the fp64 oracle on that quantity, and the HIP path may be up to 4 x as far (a different
        # but equally valid fp32 summation order); beyond that it counts as a kernel bug.
        r32 = run_oracle(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"], dtype=torch.float32)
        assert np.array_equal(r32.presence.numpy(), x["ref"].presence.numpy())
        dist = abs(float(r32.elbo_iwae) - float(x["ref"].elbo_iwae))
        bars = {"elbo_iwae": max(4.0 * dist, 1e-4 * max(abs(float(x["ref"].elbo_iwae)), 1.0))}
        m0 = run_hip(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"])
        err = abs(float(m0.elbo_iwae) - float(x["ref"].elbo_iwae))
        print("{}: elbo_iwae fp32 oracle - fp64 {:.3e}, bar {:.3e}, HIP - fp64 {:.3e}".format(case, dist, bars["elbo_iwae"], err))
        _record("forward_fp32_reference", case, quantity="elbo_iwae", fp32_oracle_distance=dist, bar=bars["elbo_iwae"], hip_error=err)
    m, ref = live_oracle_case(F, hw=hw, T=T, B=B, inputs=x, scalar_bars=bars)
    if "n_what" in FORWARD[case][5]:
        assert m.core.lib is _capi.lib(_capi.WIDE_LIB_PATH)
    want_id = ref.obj_id.numpy().reshape(T, -1, N)
    got_id = m.obj_id.cpu().numpy().reshape(T, -1, N)
    if N > 1:
        moved = PP.moved_ids(want_id)
        assert moved.sum() >= 3, "the oracle must move some object to another slot"
        assert np.array_equal(got_id[moved], want_id[moved].astype(np.float32))
        print("{}: {} (frame, row, slot) places hold an object that sat in another slot one frame earlier".format(case, int(moved.sum())))
    else:   # one slot: ids of rediscovered objects keep counting
        assert want_id.max() >= 2 and np.array_equal(got_id, want_id.astype(np.float32))
    worst = {}
    for k, v in ref.outputs.items():
        if not k.startswith("_") and k in m.outputs:
            want = v.numpy()
            got = m.outputs[k].cpu().numpy().reshape(want.shape)
            worst[k] = float(np.abs(got - want).max() / max(np.abs(want).max(), 1.0))
    _record("forward", case, gate=5e-4, oracle_margin=x["margin"], patterns=x["counts"], worst_scaled_abs_err=max(worst.values()),
            worst_output=max(worst, key=worst.get))


@pytest.mark.parametrize("case", ["K5N4T4B2_shipped_shape", "K7N3T4B5", "K2N8T3B2"])
def test_executors_agree_where_objects_vanish(case):
    """The in-launch slot chain, and the specialised instantiations on / off, against the plain launches on the same inputs: every
    output bit for bit (the chain's launches all completed: run_hip checks `check_chain`), eager and as a graph replay."""
    F, hw, T, B, N, x = _forward_inputs(case)
    run = lambda options, use_graph=False: run_hip(F, hw, x["P"], x["obs"], x["noise"], nums=x["d"]["nums"], options=options,
                                                   use_graph=use_graph)
    outs = lambda m: dict({k: v.detach().cpu().numpy().copy() for k, v in m.core.out.items()},
                          log_weights=m.core.log_weights.cpu().numpy().copy())
    n0 = spec_launches()
    ref = outs(run({"specialised": 0}))
    assert spec_launches() == n0
    assert np.array_equal(ref["prop_pres"], x["ref"].prop_pres.numpy()) and np.array_equal(ref["disc_pres"], x["ref"].disc_pres.numpy())
    shipped = case == "K5N4T4B2_shipped_shape"
    for name, options, use_graph in (("specialised", {"specialised": 1}, False), ("specialised, graph", {"specialised": 1}, True),
                                     ("slot_chain", {"slot_chain": 1}, False), ("slot_chain, graph", {"slot_chain": 1}, True),
                                     ("slot_chain, generic", {"slot_chain": 1, "specialised": 0}, False)):
        n0 = spec_launches()
        got = outs(run(options, use_graph))
        if "slot_chain" not in options:
            assert (spec_launches() - n0 > 0) == shipped, name   # k_compact<true> / k_crop_row<true, .> only for the shipped shape
        assert set(got) == set(ref)
        for k, v in ref.items():
            assert np.array_equal(v, got[k], equal_nan=True), (case, name, k)


# name: (K, N, T, B, flags, options, runs on the wide library)
BACKWARD = {
    "K5N4T4B2": (5, 4, 4, 2, {}, None, False),
    "K5N4T4B2_slot_chain": (5, 4, 4, 2, {}, {"slot_chain": 1}, False),
    "K3N3T3B3": (3, 3, 3, 3, {}, None, False),
    "K3N3T3B3_lstm": (3, 3, 3, 3, LSTM3, None, False),
    "K3N3T3B3_wide_n_what_64": (3, 3, 3, 3, dict(n_what=64), None, True),    # the only route to the wide k_compact_bwd in a full pass
    "K2N8T3B2": (2, 8, 3, 2, {}, None, False),
}


@pytest.mark.parametrize("case", sorted(BACKWARD))
def test_full_backward_where_objects_vanish(case):
    """Every parameter's gradient against autograd through the fp64 oracle at the bars of tests/pass_cases.py (TIGHT /
    LOOSE, `ill_scale=True` as the other non-shipped regimes), in cases whose later frames' gradients flow back through real
    permutations (`hole_before_last`)."""
    K, N, T, B, flags, options, wide = BACKWARD[case]
    report, ref, core = full_backward_case(K, N, T, B, (50, 50), seed=11, flags=dict(VANISH, **flags), options=options)
    # (the oracle's layouts; the HIP presences have already been asserted equal to them inside the helper)
    PP.require(ref.pattern_counts, **MINIMUMS)
    assert (core.lib is _capi.lib(_capi.WIDE_LIB_PATH)) == wide
    lw = core.out["log_weights_per_timestep"].cpu().numpy()
    want = ref.log_weights_per_timestep.detach().numpy()
    assert np.abs(lw - want).max() <= 1e-4 * np.abs(want).max()
    gmax = max(s for _, _, s in report)
    by = {n: s for n, _, s in report}
    rel = {n: e / max(max(s, by[n.replace("scale_offset", "l2.b")]) if n.endswith("transform.scale_offset") else s, 1e-4 * gmax)
           for n, e, s in report}
    _record("backward", case, tight=5e-4, patterns=ref.pattern_counts, worst_rel_err=max(rel.values()), worst_parameter=max(rel, key=rel.get))
    check_report(report, ill_scale=True)


def test_stream_chunks_cut_right_after_a_hole():
    """Chunked passes against the whole pass, bit for bit, with a chunk boundary directly after a frame in which compaction moved a
    propagated object (the carried blob then holds a permuted layout), picked from the ORACLE's pattern table; chunk size 1; the
    same through SqairStream's captured graph; and a reset of one lane leaves the other lanes' ids (everything of theirs) alone."""
    K, N, T, B, hw = 3, 3, 6, 4, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N, **VANISH)
    x = live_oracle_inputs(F, hw, T, B)
    PP.require(x["counts"], **MINIMUMS)
    pat = PP.classify_outputs(x["ref"].outputs, N)
    holes = np.flatnonzero(pat["hole"][:T - 1].any(1))           # frames (not the last) with a hole in some row
    assert len(holes) >= 1
    obs, noise = x["obs"], x["noise"]
    core = SqairCore(F, hw)
    core.set_params(x["P"])
    whole = one_pass(core, obs, noise)
    assert np.array_equal(whole["prop_pres"], x["ref"].prop_pres.numpy()) and np.array_equal(whole["disc_pres"], x["ref"].disc_pres.numpy())
    assert np.array_equal(whole["obj_id"], x["ref"].obj_id.numpy().astype(np.float32))
    R = B * K
    cuts = [[int(t) + 1, T - int(t) - 1] for t in holes] + [[1] * T]
    print("chunk boundaries after the holed frames", holes.tolist(), "->", cuts)
    for sizes in cuts:
        enc, dec = switches(T, sizes, B, R, N, hw)
        assert not enc and not dec, "the shapes of this case keep every once-per-pass layer on one kernel"
        got, _ = chunked(core, obs, noise, sizes)
        compare(got, whole)
    # the captured one-frame graph, the state updated in place
    names = ("what", "where", "presence", "obj_id", "log_weights_per_timestep")
    c2 = SqairCore(F, hw)
    c2.set_params(x["P"])
    st = SqairStream(c2, B, frames_per_step=1, use_graph=True)
    steps = [{k: v.cpu().numpy() for k, v in st.step(obs[t:t + 1], noise=noise[t:t + 1]).items()} for t in range(T)]
    for k in names:
        assert np.array_equal(np.concatenate([s[k] for s in steps]), whole[k]), k
    st.close()
    # reset lane `lane` right after the first holed frame: its rows start fresh, the others carry on bit for bit
    t_reset, lane = int(holes[0]) + 1, 1
    rows = np.arange(R) // K == lane
    c3 = SqairCore(F, hw)
    c3.set_params(x["P"])
    st = SqairStream(c3, B, frames_per_step=1, use_graph=True)
    steps = []
    for t in range(T):
        if t == t_reset:
            st.reset([lane])
        steps.append({k: v.cpu().numpy() for k, v in st.step(obs[t:t + 1], noise=noise[t:t + 1]).items()})
    st.close()
    for k in names:
        got = np.concatenate([s[k] for s in steps])
        assert np.array_equal(got[:, ~rows], whole[k][:, ~rows]), k
        assert np.array_equal(got[:t_reset, rows], whole[k][:t_reset, rows]), k
    # the reset lane starts fresh: in its first frame every object is a new discovery, numbered from 0 like a sequence's first frame
    first = steps[t_reset]["obj_id"][0][rows]
    assert ((first == -1) | ((first >= 0) & (first < N))).all(), first
    assert np.array_equal(np.sort(first[first >= 0]), np.sort(np.concatenate([np.arange((r >= 0).sum()) for r in first])))


FORECASTS = {
    "gru": (dict(k_particles=3, n_steps_per_image=3), (32, 40), 3, 4, 6),
    "lstm": (dict(k_particles=3, n_steps_per_image=2, time_transition="LSTM", prior_transition="LSTM"), (32, 40), 2, 4, 6),
    # (the random-walk prior's presence logit follows the posterior's logit of the frame before: with `prop_prior_step_bias` alone
    #  nothing vanishes in six frames -- measured on the reference rollout: 0 objects -- so this case lowers `prop_step_bias` too)
    "rw": (dict(k_particles=3, n_steps_per_image=3, prop_prior_type="rw", prop_step_bias=0.0), (32, 40), 2, 4, 6),
}


@pytest.mark.parametrize("case", sorted(FORECASTS))
def test_forecast_where_objects_vanish(case):
    """The `gru`, `lstm` and `rw` cases of tests/test_forecast.py with `prop_prior_step_bias = 0.0`, six frames, against the fp64
    rollout at that file's gate.  Required from the reference rollout alone: at least 3 objects vanish during the forecast and at
    least one survivor is moved forward over a vacated slot.  `expected_count` agrees with the reference and never increases
    (discovery is empty in a forecast)."""
    flags, hw, B, S, Fn = FORECASTS[case]
    flags = dict(flags, prop_prior_step_bias=0.0)
    K, N = flags["k_particles"], flags["n_steps_per_image"]
    seen = {}

    def require(ref, state):
        pres = np.concatenate([state.z[2].squeeze(-1).numpy()[None], ref["presence"].numpy()])     # frame -1 = the streamed state
        ids = np.concatenate([state.prev_ids.squeeze(-1).numpy()[None], ref["obj_id"].numpy()])
        n = pres.sum(-1)
        assert (n[1:] <= n[:-1]).all(), "a forecast discovers nothing"
        seen.update(vanished=int((n[:-1] - n[1:]).sum()), moved=int(PP.moved_ids(ids)[1:].any(-1).sum()))
        print("forecast {}: {} objects vanish, {} (frame, row) cells compact a hole".format(case, seen["vanished"], seen["moved"]))
        assert seen["vanished"] >= 3 and seen["moved"] >= 1, seen

    got, ref = rollout_case(case + ", prop_prior_step_bias 0", flags, hw, B, S, Fn, require=require)
    # expected_count: the weighted number of present slots per lane, against the reference's presences under the stream's weights
    cnt = ref["presence"].numpy().reshape(Fn, B, K, N).sum(-1)
    want = np.einsum("bk,fbk->fb", got["weights"].astype(np.float64), cnt)
    assert np.abs(got["expected_count"] - want).max() <= 1e-5 * max(1.0, np.abs(want).max())
    assert (np.diff(got["expected_count"], axis=0) <= 1e-6).all(), "expected_count must not increase: discovery is empty"
    moved = PP.moved_ids(np.concatenate([ref["obj_id"].numpy()[:1], ref["obj_id"].numpy()]))[1:]
    assert np.array_equal(got["obj_id"][moved], ref["obj_id"].numpy()[moved].astype(np.float32))


def test_stream_training_chunk_two_starts_from_a_holed_layout():
    """The chunk-two case of tests/test_stream_train.py (imported rows, one lane reset, every gradient against `tbptt_ref` at that
    file's bar) with objects vanishing: the first chunk's LAST frame compacts a hole in an imported row, so chunk 2 starts from a
    permuted layout, and chunk 2 itself meets the minimums -- both required from the oracle's outputs."""
    K, N, B, T = 3, 3, 3, 3

    def require(out1, out2):
        first, second = PP.classify_outputs(out1, N), PP.classify_outputs(out2, N)
        print("chunk 1:", PP.table(PP.count(first)))
        print("chunk 2:", PP.table(PP.count(second)))
        assert first["hole"][T - 1, :(B - 1) * K].any(), "the last frame of chunk 1 must compact a hole in a row that chunk 2 imports"
        PP.require(PP.count(second), **MINIMUMS)

    chunk_two_case(dict(k_particles=K, n_steps_per_image=N, **VANISH), None, False, require=require)


def test_history_tracks_follow_the_id_through_a_permutation():
    """A tests/test_history.py-style case (one frame per step, a ring of the last L steps, `tracks()` against tests/history_ref.py bit
    for bit) in which, inside the lag window, the ORACLE moves an object to another slot: `track_where` / `track_present` must
    follow the id, not the slot."""
    from tests import history_ref as H
    K, N, T, B, hw = 3, 3, 6, 4, (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N, **VANISH)
    x = live_oracle_inputs(F, hw, T, B)
    PP.require(x["counts"], **MINIMUMS)
    want_id = x["ref"].obj_id.numpy().reshape(T, B * K, N)
    moved = PP.moved_ids(want_id)
    L = lag = 4
    assert moved[T - lag:].any(), "inside the lag window some id must change its slot (oracle)"
    core = SqairCore(F, hw)
    core.set_params(x["P"])
    st = SqairStream(core, B, outputs=OUTS, history=L)
    rec = H.Recorder(B * K)
    for t in range(T):
        parent = st.carried.pending().copy()
        history_push(rec, parent, host(st.step(x["obs"][t:t + 1], noise=x["noise"][t:t + 1])))
        got = history_check(st, rec, "last", max_tracks=4 * N)
    st.close()
    assert np.array_equal(got["obj_id"], want_id[T - lag:].astype(np.float32)), "the traced ids are the oracle's"
    followed = 0
    for f, r, j in np.argwhere(moved[T - lag:]):
        if f == 0:
            continue                                   # (its previous frame is outside the window)
        oid = int(got["obj_id"][f, r, j])
        before = int(np.flatnonzero(got["obj_id"][f - 1, r] == oid)[0])
        assert before != j
        (m,) = np.flatnonzero(got["track_id"][r] == oid)
        assert got["track_present"][f, r, m] == 1 and got["track_present"][f - 1, r, m] == 1
        assert H.same_bits(got["track_where"][f, r, m], got["where"][f, r, j])
        assert H.same_bits(got["track_where"][f - 1, r, m], got["where"][f - 1, r, before])
        assert not H.same_bits(got["where"][f - 1, r, j], got["where"][f - 1, r, before])
        followed += 1
    print("tracks followed {} slot changes inside the last {} frames".format(followed, lag))
    assert followed >= 1
