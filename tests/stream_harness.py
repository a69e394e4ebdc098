"""The harness of the GPU tests that drive SqairStream, StreamTrainer and whole passes with a carried state (tests/test_*_stream.py,
test_history.py, test_track_lane.py, test_stream_state.py, test_forecast*.py, test_missing.py, test_smc_oracle.py, test_*_train.py and
the cases tests/test_presence_paths.py, test_regime_paths.py and test_latent_regimes.py run again elsewhere): the clip, parameters and
noise of a case, cores and streams on them, host copies of what a stream returns, three equality judges named by what they compare,
a stepping loop, the truth cut from an unscored run, passes with a carried state and the training step.  The cases more than one file
runs are tests/stream_cases.py.  Importable without a GPU; nothing is kept on the device between calls, so the files stay independent
of their order.

What a test expects -- its flags, batch, seeds, output lists it alone uses, keyword groups of its streams, tolerances, the reference it
is held to -- stays with the test and is stated there in full; what is here is how it obtains the thing it judges.  Asserts here are
not rewritten by pytest, so each carries what it compared."""
import math
import types

import numpy as np
import torch

from sqair_amd import _capi
from sqair_amd.data import make_sequences, to_float
from sqair_amd.flags import make_flags
from sqair_amd.model import SqairCore
from sqair_amd.stream import SqairStream
from tests import history_ref as H
from tests import idf_ref
from tests import score_ref
from tests.hip_util import draw_noise, params32
from tests.smc_ref import accumulate  # noqa: F401  (a_k as the kernel forms it: the carried log weight plus the pass's frames, in fp32)

OUTS = ("what", "where", "presence", "obj_id", "log_weights_per_timestep")
SMC_OUTS = ("ess", "resampled", "log_evidence", "ancestors")
EST_KEYS = {"best_row", "weights", "ess", "count_prob", "expected_count", "map_count", "presence", "obj_id", "where", "what", "box",
            "support", "box_mean"}
# the score family (tests/test_score_stream.py, test_idf_stream.py, test_hota_stream.py, test_match_stream.py, test_capture_effects.py):
# the frame, the batch, G truth slots for N objects, the IoU every threshold of theirs uses; FLAGS is the score's own K = 3
SCORE = types.SimpleNamespace(HW=(50, 50), FLAGS=dict(k_particles=3, n_steps_per_image=3), B=4, G=4, N=3, IOU=0.5)
IDF_IDS = 6      # P, the id columns of the IDF1 table those files ask for


# ------------------------------------------------------------------------------------------------ clip, parameters, noise
def noise(F, rng, T, R):
    return draw_noise(rng, T, R, int(F.n_steps_per_image), 4 + int(F.n_what) + 1)


def setup(flags, B, T, hw, seed=11, edits=None, obs=None, **sequences):
    """(F, P, obs, noise) of a case: make_sequences(seed) (or the caller's frames), parameters of seed 3 with jitter 0.05 around the
    clip's mean image, noise from default_rng(seed + 1).  edits: names of tests/latent_regimes.EDITS applied to the parameters."""
    F = make_flags(**flags)
    if obs is None:
        obs = to_float(make_sequences(B, T=T, canvas=hw, seed=seed, **sequences)["imgs"])
    P = params32(F, hw, 3, 0.05, obs.mean((0, 1)))
    if edits:
        from tests import latent_regimes
        P = latent_regimes.apply_edits(P, F, edits)
    return F, P, obs, noise(F, np.random.default_rng(seed + 1), T, B * int(F.k_particles))


def core(F, hw, P, options=None, lib_path=None):
    c = SqairCore(F, hw, lib_path=lib_path, options=options)
    c.set_params(P)
    return c


def stream(core_or_parts, B, **kw):
    """A SqairStream on a core, or on a new core of (F, hw, P)."""
    return SqairStream(core_or_parts if isinstance(core_or_parts, SqairCore) else core(*core_or_parts), B, **kw)


# ------------------------------------------------------------------------------------------------ host copies
def _numpy(x):
    return {k: _numpy(v) for k, v in x.items()} if isinstance(x, dict) else x.cpu().numpy()


def host(out):
    """What a stream returned, on the host: dicts of any depth of numpy arrays, after a synchronise."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return _numpy(out)


# ------------------------------------------------------------------------------------------------ judges
def words(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _raw(a):
    """Anything a stream returns as the bytes it holds (NaN == NaN, -0.0 != 0.0)."""
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(a)).view(np.uint8)


def _bits_equal(x, y):
    return np.array_equal(words(x), words(y))


def _values_equal(x, y):
    return np.array_equal(x, y, equal_nan=True)


def _bytes_equal(x, y):
    if tuple(np.shape(x)) != tuple(np.shape(y)):
        return False
    x, y = _raw(x), _raw(y)
    return x.shape == y.shape and np.array_equal(x, y)


def differ(x, y):
    """For an assert's message: dtypes and shapes of the two, and the first entries that differ."""
    x, y = (np.asarray(v.detach().cpu() if isinstance(v, torch.Tensor) else v) for v in (x, y))
    what = "{} {} against {} {}".format(x.dtype, x.shape, y.dtype, y.shape)
    if x.shape != y.shape:
        return what
    at = np.argwhere(~((x == y) | ((x != x) & (y != y))) | (np.signbit(x) != np.signbit(y)) if x.dtype.kind == "f" else x != y)[:4]
    return what + ", first at " + "; ".join("{}: {!r} {!r}".format(tuple(i), x[tuple(i)], y[tuple(i)]) for i in at.tolist())


def _judge(equal, a, b, keys, where, path=""):
    at = lambda k: (where, path + k)
    if keys is None:
        assert set(a) == set(b), (at(""), sorted(set(a) ^ set(b)))
        keys = a
    for k in keys:
        if isinstance(a[k], dict):
            _judge(equal, a[k], b[k], None, where, path + k + ".")
        else:
            assert equal(a[k], b[k]), (at(k), differ(a[k], b[k]))


def same_bits(a, b, keys=None, where=()):
    """float32 as 32-bit words (-0.0 is not 0.0, a NaN equals only the same NaN), other dtypes by value -- over `keys` of the two
    dicts, or over all of them, which must then be the same ones, dicts inside included."""
    _judge(_bits_equal, a, b, keys, where)


def same_values(a, b, keys=None, where=()):
    """By value, any NaN equal to any NaN (-0.0 equals 0.0); the keys as same_bits takes them."""
    _judge(_values_equal, a, b, keys, where)


def same_bytes(a, b, keys=None, where=()):
    """Shape and raw bytes, whatever the dtype, of arrays and tensors; the keys as same_bits takes them."""
    _judge(_bytes_equal, a, b, keys, where)


# ------------------------------------------------------------------------------------------------ stepping
def run(st, obs, noise, Ts=1, before=None, **per_step):
    """Steps ``st`` through the clip, Ts frames a step; returns the host copies of every step's outputs.  ``before(s)``: called ahead
    of step s.  per_step: step() keywords, ``observed`` by frame, everything else one entry per step (None: left out of that call)."""
    outs = []
    for s in range(obs.shape[0] // Ts):
        if before is not None:
            before(s)
        f = slice(s * Ts, (s + 1) * Ts)
        kw = {k: (v[f] if k == "observed" else v[s]) for k, v in per_step.items() if v is not None}
        kw = {k: v for k, v in kw.items() if v is not None}
        outs.append(host(st.step(obs[f], noise=noise[f], **kw)))
    return outs


def carried_in(st):
    """The log weights the next step's rows carry into it: log_weight_sum through the pending source map (a reset or resample armed
    on the host; with SMC the device buffers already hold it)."""
    lw = st.log_weight_sum.cpu().numpy()
    m = st.carried.pending()
    return np.where(m >= 0, lw[np.maximum(m, 0)], np.float32(0.0)).astype(np.float32)


def cap(counts, skipped="skipped"):
    """Prints a run's counts; decisions were made, and at most 1 % of them were left out as within the fp32 band of a threshold."""
    print(counts)
    assert counts["decisions"] > 0 and counts[skipped] <= 0.01 * counts["decisions"], counts


# ------------------------------------------------------------------------------------------------ truth from an unscored run
def make_truth(outs, Ts, seed=7):
    """One ``truth`` dict per step from an unscored run's lane boxes, on the score family's shapes: the boxes jittered by 1.5 px, put
    into the G truth slots by a rotation that changes every four frames, a fifth of them dropped, a truth added in the spare slot in a
    third of the frames, a tenth of the frames without a valid truth."""
    B, G, N = SCORE.B, SCORE.G, SCORE.N
    rng = np.random.default_rng(seed)
    truth = []
    for s, o in enumerate(outs):
        lane = o["lane"]
        box = np.zeros((Ts, B, G, 4), np.float32)
        present = np.zeros((Ts, B, G), np.int32)
        for f in range(Ts):
            shift = ((s * Ts + f) // 4) % 2
            for b in range(B):
                for j in range(N):
                    g = (j + shift) % N
                    box[f, b, g] = lane["box"][f, b, j] + 1.5 * rng.standard_normal(4)
                    present[f, b, g] = lane["presence"][f, b, j] != 0 and rng.uniform() < 0.8
                if rng.uniform() < 0.33:
                    box[f, b, N], present[f, b, N] = (rng.uniform(0, 30), rng.uniform(0, 30), 12.0, 12.0), 1
        valid = (rng.uniform(size=(Ts, B)) < 0.9).astype(np.int32)
        truth.append(dict(box=box, present=present, valid=valid))
    return truth


def unscored_truth(st, obs, noise, Ts=1, observed=None, cut=make_truth):
    """Runs the unscored stream ``st`` through the clip and closes it; returns (cut(outs, Ts), outs)."""
    outs = run(st, obs, noise, Ts, observed=observed)
    st.close()
    return cut(outs, Ts), outs


class IdfRef(object):
    """The IDF1 reference (tests/idf_ref.py) carried along a stream of the score family: the table, fed every step's own lane outputs."""

    def __init__(self, ids="obj_id"):
        self.table, self.ids = idf_ref.new_table(SCORE.B, SCORE.G, IDF_IDS), ids

    def step(self, o, truth):
        lane = o["lane"]
        words = score_ref.words(lane["obj_id"]) if self.ids == "obj_id" else lane["lane_id"]
        near = 4.0 * score_ref.iou32_error(truth["box"] * (truth["present"] != 0)[..., None], lane["box"])
        first = idf_ref.fragile_from(score_ref.iou_table(truth["box"], lane["box"]), lane["presence"], lane["map_count"], truth["present"],
                                     truth["valid"], SCORE.IOU, near)
        assert near < 1e-5 and (first == lane["map_count"].shape[0]).all(), ("a pair within the fp32 error of the threshold", near, first)
        self.table = idf_ref.accumulate(self.table, lane["box"], lane["presence"], words, lane["map_count"], truth["box"], truth["present"],
                                        truth["valid"], lane["truth_match"], SCORE.IOU)

    def close(self, lanes):
        mask = np.zeros(SCORE.B, np.int32)
        mask[lanes] = 1
        self.table, _ = idf_ref.solve(self.table, close=mask)

    def check_table(self, st):
        used = self.table["col_id"] >= 0
        for n in _capi.IDF_TABLE + ("totals",):
            got, want = st._idf[n].cpu().numpy(), self.table[n]
            if n == "overlap":      # (the words of a free column are never read)
                got, want = np.where(used[:, None, :], got, 0), np.where(used[:, None, :], want, 0)
            if n == "col_frames":
                got, want = np.where(used, got, 0), np.where(used, want, 0)
            assert np.array_equal(got, want), (n, got, want)

    def check_score(self, got):
        _, open_ = idf_ref.solve(self.table)
        per_lane = self.table["totals"] + open_
        for i, n in enumerate(idf_ref.TOTALS):
            key = "frag_per_lane" if n == "frag" else n
            assert got[key].dtype == torch.int64 and np.array_equal(got[key].numpy(), per_lane[:, i]), (n, got[key], per_lane[:, i])
        idtp = idf_ref.TOTALS.index("idtp")
        assert got["assign"].dtype == torch.int32, got["assign"].dtype
        for b in range(SCORE.B):
            idf_ref.check_assign(self.table, b, got["assign"][b].numpy(), int(open_[b, idtp]))
        for n, v in idf_ref.pooled(per_lane).items():
            assert got[n] == v or (np.isnan(got[n]) and np.isnan(v)), (n, got[n], v)
        return dict(zip(idf_ref.TOTALS, per_lane.sum(0).tolist()))


# ------------------------------------------------------------------------------------------------ the track history
FIELD_OF = dict(where="where", presence="presence", obj_id="obj_id", what="what", log_w="log_weights_per_timestep")


def history_push(rec, parent, o, fields=tuple(FIELD_OF)):
    rec.push(parent, **{k: o[FIELD_OF[k]] for k in fields})


def history_check(st, rec, start, start_rows=None, lag=None, max_tracks=None, table=True, fields=tuple(FIELD_OF)):
    """tracks() of `st` against the reference tracer over the steps recorded in `rec`; returns the device's result."""
    got = host(st.tracks(lag=lag, start=start, max_tracks=max_tracks, table=table))
    lag = st.history if lag is None else lag
    N = st.core.N
    M = (2 * N if max_tracks is None else max_tracks) if table else None
    if rec.steps:
        want = H.trace(rec.steps, st.history, lag, st.K, None if start == "last" else start_rows, M)
    else:
        want = H.empty_trace(st.T, st.R, N, st.core.nw, lag, st.K, fields, M)
    assert set(want) <= set(got), sorted(set(want) - set(got))
    for k, v in want.items():
        assert got[k].dtype == v.dtype and H.same_bits(got[k], v), (k, start, lag, got[k].dtype, v.dtype, np.argwhere(got[k] != v)[:4])
    assert ("weights" in got) == (start == "next") and ("track_id" in got) == bool(table), (start, table, sorted(got))
    return got


# ------------------------------------------------------------------------------------------------ passes with a carried state
PER_FRAME = [n for n in _capi.OUTPUT_FIELDS if not n.startswith("final_")]
FINAL = [n for n in _capi.OUTPUT_FIELDS if n.startswith("final_")]
GATE = 2e-5    # the repository's per-output gate (scaled absolute error), for decoder outputs whose dense kernel changes with T
MT_ROWS, T2_ROWS, T2_KC = 6000, 512, 40   # once-per-pass layers: kernel (summation order) by row count (csrc/sqair_linear.hip)


def _ptr(t):
    return None if t is None else t.data_ptr()


def set_state(core, B, state_in=None, state_out=None, src=None):
    nb = core.lib.sqair_state_bytes(core.handle, B) if (state_in is not None or state_out is not None) else 0
    core.check(core.lib.sqair_set_state(core.handle, _ptr(state_in), _ptr(state_out), _ptr(src), nb, B), "sqair_set_state")


def blob(core, B):
    return torch.zeros(core.lib.sqair_state_bytes(core.handle, B) // 4, dtype=torch.float32, device=core.device)


def one_pass(core, obs, noise, state_in=None, state_out=None, src=None, t_offset=0):
    """One eager pass of len(obs) frames (state as given; none = the handle's plain pass); every output, on the host."""
    T, B = obs.shape[:2]
    core.bind(T, B, "all")
    with core.on_stream():
        core.obs.copy_(torch.as_tensor(obs))
        core.noise.copy_(torch.as_tensor(noise).reshape(core.noise.shape))
        set_state(core, B, state_in, state_out, src)
        core.check(core.lib.sqair_forward(*core._args(t_offset)), "sqair_forward")
    core.stream.synchronize()
    if core.options.get("slot_chain"):
        core.check_chain()
    return {k: v.cpu().numpy().copy() for k, v in core.out.items()}


def chunked(core, obs, noise, sizes, src_before=None):
    """The same frames as passes of `sizes` frames, the state carried in place; src_before: {chunk index: source map}."""
    B = obs.shape[1]
    state = blob(core, B)
    outs, t0 = [], 0
    for i, c in enumerate(sizes):
        src = None
        if src_before and i in src_before:
            src = torch.as_tensor(np.asarray(src_before[i], dtype=np.int32), device=core.device)
        outs.append(one_pass(core, obs[t0:t0 + c], noise[t0:t0 + c], None if i == 0 else state, state, src))
        t0 += c
    merged = {k: np.concatenate([o[k] for o in outs]) for k in PER_FRAME}
    merged.update({k: outs[-1][k] for k in FINAL})
    return merged, outs


def switches(T, sizes, B, R, N, hw):
    """Whether a once-per-pass layer runs another dense kernel in the whole pass than in some chunk: (encoder, decoder)."""
    kc = math.ceil(hw[0] * hw[1] / 16)
    enc = kc >= T2_KC and any((c * B >= T2_ROWS) != (T * B >= T2_ROWS) for c in sizes)
    dec = any((c * R * N >= MT_ROWS) != (T * R * N >= MT_ROWS) for c in sizes)
    return enc, dec


def compare(got, want, loose=()):
    """Every output of two passes: by value (NaN equal to NaN), those in `loose` within GATE."""
    for k in PER_FRAME + FINAL:
        if k in loose:
            scale = max(float(np.abs(want[k]).max()), 1.0)
            err = float(np.abs(got[k] - want[k]).max()) / scale
            assert err <= GATE, (k, err)
        else:
            assert np.array_equal(got[k], want[k], equal_nan=True), (k, float(np.abs(got[k] - want[k]).max()))


# ------------------------------------------------------------------------------------------------ against the fp64 oracle
def scaled(got, want):
    got = np.asarray(got, np.float64).reshape(want.shape)
    return float(np.abs(got - want).max() / max(1.0, float(np.abs(want).max())))


def frames(hw, B, T, seed):
    if min(hw) < 20:   # (the sprite generator needs room for its objects: plain random frames)
        return np.random.default_rng(seed).uniform(size=(T, B) + tuple(hw)).astype(np.float32)
    return to_float(make_sequences(B, T=T, canvas=hw, seed=seed)["imgs"])


# ------------------------------------------------------------------------------------------------ training with a carried state
def train_setup(flags, B, T, hw, seed, edits=None):
    """(F, obs, P) of a training case: one or two small objects, the parameters held (lr 0: the optimiser step changes nothing)."""
    F, P, obs, _ = setup(dict(learning_rate=0.0, **flags), B, T, hw, seed, edits=edits, n_objects=(1, 2), obj_size=10)
    return F, obs, P


def train_step(tr, *args, **kw):
    """StreamTrainer.step is asynchronous on its core's stream: wait for it, return the gradient on the host."""
    g = tr.step(*args, **kw)
    torch.cuda.synchronize()
    return g.cpu().numpy()


def gclose(got, want, tol):
    got, want = np.asarray(got), np.asarray(want)
    err = float(np.abs(got - want).max())
    assert err <= tol * float(np.abs(want).max()), (err, float(np.abs(want).max()))


def chunks(F, obs, B, T, n, seed=5):
    rng = np.random.default_rng(seed)
    R = B * int(F.k_particles)
    return [(obs[i * T:(i + 1) * T], noise(F, rng, T, R)) for i in range(n)]


