"""-m gpu: whole object forecasts (include/sqair_hip.h: sqair_forecast_fan; SqairStream.forecast(samples=, lane=)) at the smallest
shapes that still exercise every path: B = 2-3, K = 3-4, N = 3, F = 3, 32 x 40 frames, S in {1, 4}.

At these shapes every dense launch -- the decoder's F * R * S * N = 432 rows included -- stays below the 1792-row boundary of
sq_launch_linear, so both sides of every bitwise comparison below (a fan against plain forecasts of a quarter of its rows) pick the
same dense kernels: equal bits are then a statement about the fan-out, not about kernel selection."""
import ctypes as C

import numpy as np
import pytest
import torch

from sqair_amd import _capi
from sqair_amd.data import make_sequences, to_float
from sqair_amd.flags import make_flags
from sqair_amd.stream import SqairStream
from tests import forecast_lane_check as FC
from tests import forecast_lane_ref as FL
from tests.hip_util import draw_noise, params32
from tests.stream_harness import core as make_core, host, same_bits

pytestmark = pytest.mark.gpu

HW, B, K, N, FN = (32, 40), 3, 4, 3, 3
R = B * K
FLAGS = dict(k_particles=K, n_steps_per_image=N)
PER_ROW = ("what", "where", "presence", "presence_prob", "presence_logit", "obj_id", "canvas", "glimpse")


def _core(P=None, **kw):
    F = make_flags(**FLAGS)
    return F, make_core(F, HW, params32(F, HW, 3, 0.05) if P is None else P, **kw)


def _obs(T, seed=19):
    return to_float(make_sequences(B, T=T, canvas=HW, seed=seed)["imgs"])


def _step_noise(T, seed):
    """Step noise whose presence uniforms are small: objects are discovered and kept, so the forecasts have something to follow."""
    noise = draw_noise(np.random.default_rng(seed), T, R, N, 4 + 50 + 1)
    noise[..., -1] *= 0.3
    return noise


def _stream(T=2, **kw):
    F, core = _core()
    st = SqairStream(core, B, frames_per_step=T, use_graph=False, **kw)
    return F, core, st


def _raw(st, S, noise, src, log_w=None, fan=True, lane=False, capture=False):
    """sqair_forecast_fan (fan) or sqair_forecast on caller buffers with the stream's handle and state: {name: device tensor}."""
    core = st.core
    RS = R * S
    z = lambda *shp: torch.zeros(shp, dtype=torch.float32, device=core.device)
    out = dict(what=z(FN, RS, N, core.nw), where=z(FN, RS, N, 4), presence=z(FN, RS, N), presence_prob=z(FN, RS, N),
               presence_logit=z(FN, RS, N), obj_id=z(FN, RS, N), canvas=z(FN, RS, *HW), glimpse=z(FN, RS, N, core.G, core.G),
               mean_canvas=z(FN, B, *HW), expected_count=z(FN, B))
    c_out = _capi.SqairForecastOutputs(**{k: v.data_ptr() for k, v in out.items()})
    c_out.log_w = None if log_w is None else log_w.data_ptr()
    lo, c_lane = {}, None
    if lane:
        shapes = _capi.forecast_lane_shapes(FN, B, K, N)
        lo = {n: torch.full(shp, -7, dtype=torch.int32 if n in _capi.FORECAST_LANE_INT_FIELDS else torch.float32, device=core.device)
              for n, shp in shapes.items()}
        c_lane = C.byref(_capi.SqairForecastLane(iou_min=0.5, **{n: t.data_ptr() for n, t in lo.items()}))
    nb = core.lib.sqair_forecast_fan_workspace_bytes(core.handle, FN, B, S) if fan else core.lib.sqair_forecast_workspace_bytes(core.handle, FN, B)
    ws = z(nb // 4)
    nz = torch.as_tensor(noise, dtype=torch.float32, device=core.device).contiguous()
    s = torch.cuda.Stream(device=core.device)
    s.wait_stream(torch.cuda.current_stream())
    ss = C.c_void_p(s.cuda_stream)
    head = (core.handle, core.flat.data_ptr(), core.packed.data_ptr(), nz.data_ptr(), FN, B)
    srcp = None if src is None else src.data_ptr()
    if fan:
        call = lambda: core.check(core.lib.sqair_forecast_fan(*head, S, srcp, C.byref(c_out), c_lane, ws.data_ptr(), nb, ss), "sqair_forecast_fan")
    else:
        call = lambda: core.check(core.lib.sqair_forecast(*head, srcp, C.byref(c_out), ws.data_ptr(), nb, ss), "sqair_forecast")
    if capture:
        core.check(core.lib.sqair_capture_begin(core.handle, ss), "sqair_capture_begin")
        call()
        assert core.lib.sqair_capture_end(core.handle, ss, 3) > 0
        for v in list(out.values()) + list(lo.values()):
            v.fill_(-7)
        torch.cuda.synchronize()
        core.check(core.lib.sqair_capture_launch(core.handle, 3, ss), "sqair_capture_launch")
    else:
        call()
    s.synchronize()
    out.update({"lane." + n: t for n, t in lo.items()})
    return out


@pytest.fixture(scope="module")
def stepped():
    """A stream after two frames, a source map with a fresh row and a repeated one, non-uniform log weights, one noise draw for S = 4."""
    F, core, st = _stream()
    st.step(_obs(2), noise=_step_noise(2, 11))
    torch.cuda.synchronize()
    rng = np.random.default_rng(4)
    src = np.arange(R, dtype=np.int32)
    src[1], src[5], src[6] = -1, 4, R + 3      # fresh, a repeated row, out of range (fresh)
    src = torch.as_tensor(src, device=core.device)
    lw = torch.as_tensor(rng.normal(0, 2, R).astype(np.float32), device=core.device)
    noise = draw_noise(rng, FN, R * 4, N, core.nzw)
    noise[..., 0, :, -1] *= 0.5                # (objects that live on for a few frames)
    return st, src, lw, noise


def test_s1_without_lane_is_sqair_forecast(stepped):
    st, src, lw, noise = stepped
    n1 = noise[:, :R]
    for m in (src, None):
        a, b = host(_raw(st, 1, n1, m, lw, fan=False)), host(_raw(st, 1, n1, m, lw, fan=True))
        same_bits(a, b, list(a))
    assert a["where"].any() and a["canvas"].any()


def test_every_rollout_is_the_plain_forecast_of_its_row_and_noise(stepped):
    st, src, lw, noise = stepped
    S = 4
    fan = host(_raw(st, S, noise, src, lw))
    n5 = noise.reshape((FN, R, S) + noise.shape[2:])
    alive = 0
    for s in range(S):
        plain = host(_raw(st, 1, n5[:, :, s], src, lw, fan=False))
        for k in PER_ROW:
            got = fan[k].reshape((FN, R, S) + fan[k].shape[2:])[:, :, s]
            same_bits({k: got}, plain, [k], s)
        alive += int(plain["presence"].sum())
    assert alive > 0
    # the rollouts of a row differ (their noise does), and a fresh row's start from the initial state
    p = fan["where"].reshape(FN, R, S, N, 4)
    assert not np.array_equal(p[:, :, 0], p[:, :, 1])
    # summaries: weights w_k / S over the lane's K * S rows
    w = np.exp(lw.cpu().numpy().astype(np.float64).reshape(B, K))
    w = np.repeat(w / w.sum(1, keepdims=True), S, 1) / S
    cv = fan["canvas"].astype(np.float64).reshape(FN, B, K * S, -1)
    cnt = fan["presence"].astype(np.float64).reshape(FN, B, K * S, N).sum(-1)
    want_mc = np.einsum("bq,fbqp->fbp", w, cv).reshape(fan["mean_canvas"].shape)
    want_ec = np.einsum("bq,fbq->fb", w, cnt)
    assert np.abs(fan["mean_canvas"] - want_mc).max() <= 1e-5 * np.abs(want_mc).max()
    assert np.abs(fan["expected_count"] - want_ec).max() <= 1e-5 * max(1.0, np.abs(want_ec).max())
    # NULL log_w: uniform; a NaN lane: NaN summaries, the other lanes untouched
    u = host(_raw(st, S, noise, src, None))
    assert np.abs(u["expected_count"] - cnt.mean(2)).max() <= 1e-5 * max(1.0, cnt.max())
    lw2 = lw.clone()
    lw2[K + 1] = float("nan")
    e = host(_raw(st, S, noise, src, lw2))
    assert np.isnan(e["expected_count"][:, 1]).all() and np.isnan(e["mean_canvas"][:, 1]).all()
    assert np.array_equal(e["expected_count"][:, [0, 2]], fan["expected_count"][:, [0, 2]])


def test_captured_fan_replays_the_eager_call(stepped):
    st, src, lw, noise = stepped
    eager = host(_raw(st, 4, noise, src, lw, lane=True))
    graph = host(_raw(st, 4, noise, src, lw, lane=True, capture=True))
    same_bits(eager, graph, list(eager))
    assert (eager["lane.best_row"] >= 0).all() and eager["lane.presence"].sum() > 0


def _check_lane(st, res, S, lw):
    """res["lane"] against the reference applied to the call's own per-rollout outputs, start rows and log weights."""
    res = host(res)
    ln = res["lane"]
    ref = FL.lane_forecast(ln["start_where"], ln["start_presence"], ln["start_obj_id"], res["where"], res["presence"], res["obj_id"],
                           lw, K, S, HW, 0.5)
    margins, counts = FC.check(ln, ref, res["where"], K, S, HW, 0.5)
    FC.check_counts(ln, ref, res["presence"], K, S, margins)
    assert np.allclose(ln["weights"], res["weights"], rtol=1e-6, atol=0)
    return res, ref, counts


def _next_lw(st):
    cs, dev = st.carried, st.core.device
    with torch.cuda.device(dev):
        src, lw = cs.next_rows(torch.zeros(R, dtype=torch.int32, device=dev), torch.zeros(R, device=dev))
        torch.cuda.synchronize()
        return src.cpu().numpy().copy(), lw.cpu().numpy().copy()


@pytest.mark.parametrize("S", [1, 4])
def test_stream_lane_forecast_against_the_reference(S):
    """No SMC; after reset([1]) (lane 1 has no objects); after resample(src)."""
    F, core, st = _stream(T=1)
    obs = _obs(3)
    objects = 0
    for step in range(3):
        st.step(obs[step:step + 1], noise=_step_noise(1, 20 + step))
        if step == 1:
            st.reset([1])
        if step == 2:
            src = np.arange(R)
            src[0:K] = [2, 2, 0, 3]
            src[2 * K] = -1
            st.resample(src)
        smap, lw = _next_lw(st)
        res, ref, counts = _check_lane(st, st.forecast(FN, samples=S, lane=True), S, lw)
        assert res["where"].shape == (FN, R * S, N, 4) and res["lane"]["alive"].shape == (FN, B, N)
        # the start rows are the rows the next step starts from: the blob through the pending map
        if step == 1:
            assert not res["lane"]["start_presence"][K:2 * K].any() and not res["lane"]["presence"][1].any()
            assert not res["lane"]["support"][1].any() and not res["lane"]["alive"][:, 1].any()
        if step == 2:
            sp = res["lane"]["start_where"].reshape(B, K, N, 4)
            assert np.array_equal(sp[0, 0], sp[0, 1]) and not res["lane"]["start_presence"][2 * K].any()
        objects += int(res["lane"]["presence"].sum())
    assert objects > 0
    st.close()


@pytest.mark.parametrize("ess_frac", [0.0, 0.4])
def test_stream_lane_forecast_with_smc_and_missing(ess_frac):
    """SMC on -- ess_frac = 0: no lane ever resamples, so every lane carries non-uniform weights into the forecast; 0.4: lanes
    resample, the forecast weighs the equally weighted surviving set through the resampler's map -- and missing=True with a coasted
    lane."""
    F, core = _core()
    st = SqairStream(core, B, frames_per_step=1, use_graph=False, resample="systematic", ess_frac=ess_frac, seed=3, missing=True)
    obs = _obs(4, seed=7)
    nonuniform = objects = resampled = 0
    for step in range(4):
        st.step(obs[step:step + 1], noise=_step_noise(1, 30 + step), observed=None if step != 2 else np.array([True, False, True]))
        _, lw = _next_lw(st)
        res, ref, counts = _check_lane(st, st.forecast(FN, samples=4, lane=True), 4, lw)
        nonuniform += int((np.ptp(res["lane"]["weights"], axis=1) > 0).sum())
        resampled += int(st.resampled.cpu().numpy().sum())
        objects += int(res["lane"]["presence"].sum())
    assert objects > 0 and (nonuniform > 0 if ess_frac == 0.0 else resampled > 0), (nonuniform, resampled, objects)
    st.close()


@pytest.mark.parametrize("smc", [False, True])
def test_lane_forecasting_between_steps_changes_nothing(smc):
    """The two-stream setup of tests/test_forecast.py: a stream that calls forecast(F, samples=4, lane=True) before every step equals
    one that never forecasts, bit for bit: the step outputs, the blob's bytes, the SMC accumulators."""
    F = make_flags(**FLAGS)
    P = params32(F, HW, 3, 0.05)
    kw = dict(resample="systematic", ess_frac=0.7) if smc else {}
    (_, ca), (_, cb) = _core(P), _core(P)
    sa, sb = SqairStream(ca, B, seed=5, **kw), SqairStream(cb, B, seed=5, **kw)
    obs = _obs(5, seed=31)
    for s in range(5):
        if s == 3:
            sa.reset([1])
            sb.reset([1])
        fc = sa.forecast(FN, samples=4, lane=True)
        nz = _step_noise(1, 40 + s)
        oa, ob = host(sa.step(obs[s:s + 1], noise=nz)), host(sb.step(obs[s:s + 1], noise=nz))
        torch.cuda.synchronize()
        assert (fc["lane"]["best_row"] >= 0).all()
        for k in ob:
            assert np.array_equal(oa[k], ob[k], equal_nan=True), (s, k)
        assert torch.equal(sa.state.view(torch.int32), sb.state.view(torch.int32)), s
        assert torch.equal(sa.log_weight_sum, sb.log_weight_sum), s
        if smc:
            for k in ("log_z", "ess", "_src", "resampled", "log_evidence"):
                assert torch.equal(getattr(sa, k), getattr(sb, k)), (s, k)
        assert (sa._armed is None) == (sb._armed is None) and sa._src_is_identity == sb._src_is_identity


def test_default_arguments_are_the_plain_forecast():
    """forecast(F) and forecast(F, samples=1) draw the same Philox noise and give the same bits; samples=4 keeps the key."""
    F, core, st = _stream()
    st.step(_obs(2), noise=_step_noise(2, 11))
    a, b = host(st.forecast(FN)), host(st.forecast(FN, samples=1, lane=True))
    same_bits(a, b, list(a))
    assert "lane" in b and "lane" not in a
    with pytest.raises(ValueError):
        st.forecast(FN, samples=0)
    with pytest.raises(ValueError):
        st.forecast(FN, samples=257)
    with pytest.raises(ValueError):
        st.forecast(FN, lane=True, lane_iou=0.0)
    st.close()
