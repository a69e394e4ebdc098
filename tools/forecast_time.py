#!/usr/bin/env python
"""Cost of a forecast (include/sqair_hip.h: sqair_forecast; SqairStream.forecast) at cfg-2's batch (B = 32 sequences x K = 5
particles, N = 4, 50 x 50 frames), next to one stream step of the same batch.

For F = 1, 10, 30 frames: the sqair_forecast call alone on resident buffers (per-particle outputs and the summaries), eager (issued
each time) and as a captured graph (sqair_capture_begin / _end, replayed), each synchronous per call after a warm-up, timed with HIP
events; and SqairStream.forecast() end to end (noise fill, source map, output copies).  Reported per forecast frame and per call.
The stream step is SqairStream.step() of one frame, graph-replayed, timed the same way.

    python tools/forecast_time.py [--reps 200] [--warmup 20] [--out profiles/forecast_time.json]

With --samples S (and --lane): object forecasts (sqair_forecast_fan) instead.  At the same batch and F = 1, 10, 30 the plain forecast,
the fan of S rollouts per particle and, with --lane, the fan with the lane outputs -- three captured graphs replayed in turn, one
replay each per repetition, so that all of them see the same clocks --, then one camera (B = 1, K = 1) with S = 32.  The yardstick is
the same run's plain forecast; nothing is gated on these numbers.

    python tools/forecast_time.py --samples 8 --lane [--out profiles/forecast_lane_time.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sqair_amd import _capi  # noqa: E402
from sqair_amd.data import config_inputs, make_sequences, to_float  # noqa: E402
from sqair_amd.flags import make_flags  # noqa: E402
from sqair_amd.model import SqairCore  # noqa: E402
from sqair_amd.params import init_params  # noqa: E402
from sqair_amd.stream import SqairStream  # noqa: E402


def _time(fn, reps, warmup, stream):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    with torch.cuda.stream(stream):
        for i in range(reps):
            ev[i][0].record()
            fn()
            ev[i][1].record()
            stream.synchronize()   # (latency: each call waits for the previous one's results)
    return np.array([a.elapsed_time(b) for a, b in ev])


def _fan_graphs(core, st, B, K, N, hw, Fn, variants):
    """One captured graph per (name, S, lane) of ``variants`` on resident buffers; returns {name: (replay, nodes, buffers)}."""
    lib, ss = core.lib, core._stream()
    z = lambda *shp: torch.zeros(shp, dtype=torch.float32, device=core.device)
    graphs = {}
    for slot, (name, S, lane) in enumerate(variants):
        R = B * K * S
        out = dict(what=z(Fn, R, N, core.nw), where=z(Fn, R, N, 4), presence=z(Fn, R, N), presence_prob=z(Fn, R, N),
                   presence_logit=z(Fn, R, N), obj_id=z(Fn, R, N), canvas=z(Fn, R, *hw), glimpse=z(Fn, R, N, core.G, core.G),
                   mean_canvas=z(Fn, B, *hw), expected_count=z(Fn, B))
        c_out = _capi.SqairForecastOutputs(**{k: v.data_ptr() for k, v in out.items()})
        c_out.log_w = st.log_weight_sum.data_ptr()
        lo = {n: z(*shp) for n, shp in _capi.forecast_lane_shapes(Fn, B, K, N).items()} if lane else {}
        c_lane = C.byref(_capi.SqairForecastLane(iou_min=0.5, **{n: t.data_ptr() for n, t in lo.items()})) if lane else None
        noise = z(Fn, R, 2, N, core.nzw)
        core.check(lib.sqair_fill_noise(core.handle, noise.data_ptr(), Fn, B * S, B * S, 0, 1, 1 << 63, ss), "sqair_fill_noise")
        head = (core.handle, core.flat.data_ptr(), core.packed.data_ptr(), noise.data_ptr(), Fn, B)
        if name == "plain":
            ws = z(lib.sqair_forecast_workspace_bytes(core.handle, Fn, B) // 4)
            call = lambda head=head, c_out=c_out, ws=ws: lib.sqair_forecast(*head, st._src.data_ptr(), C.byref(c_out), ws.data_ptr(),
                                                                            ws.numel() * 4, ss)
        else:
            ws = z(lib.sqair_forecast_fan_workspace_bytes(core.handle, Fn, B, S) // 4)
            call = lambda head=head, c_out=c_out, ws=ws, S=S, c_lane=c_lane: lib.sqair_forecast_fan(
                *head, S, st._src.data_ptr(), C.byref(c_out), c_lane, ws.data_ptr(), ws.numel() * 4, ss)
        core.stream.synchronize()
        core.check(lib.sqair_capture_begin(core.handle, ss), "sqair_capture_begin")
        core.check(call(), name)
        nodes = lib.sqair_capture_end(core.handle, ss, slot)
        assert nodes > 0, nodes
        graphs[name] = (lambda slot=slot: core.check(lib.sqair_capture_launch(core.handle, slot, ss), "sqair_capture_launch"), nodes,
                        (out, lo, noise, ws))
    return graphs


def _alternate(graphs, reps, warmup, stream):
    """Each graph replayed once per repetition, in turn, synchronous per replay; {name: median ms}."""
    names = list(graphs)
    for _ in range(warmup):
        for n in names:
            graphs[n][0]()
    torch.cuda.synchronize()
    ms = {n: [] for n in names}
    with torch.cuda.stream(stream):
        for _ in range(reps):
            for n in names:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                graphs[n][0]()
                b.record()
                stream.synchronize()
                ms[n].append(a.elapsed_time(b))
    return {n: float(np.median(v)) for n, v in ms.items()}


def _fan_setup(B, K, N, hw):
    F = make_flags(k_particles=K, n_steps_per_image=N)
    obs = torch.as_tensor(to_float(make_sequences(B, T=8, canvas=hw, seed=7)["imgs"])).cuda()
    P = {k: np.asarray(v, dtype=np.float32) for k, v in
         init_params(F, hw, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    core = SqairCore(F, hw)
    core.set_params(P)
    st = SqairStream(core, B, frames_per_step=1, use_graph=True, resample="systematic", ess_frac=0.5)
    for t in range(8):
        st.step(obs[t:t + 1])
    return core, st


def fan_main(args):
    ov, _, _, _ = config_inputs(2)
    B, K, N, hw = 32, int(ov["k_particles"]), int(ov["n_steps_per_image"]), (50, 50)
    S = args.samples
    res = dict(build_id=_capi.build_id(), device=torch.cuda.get_device_name(0), N=N, hw=list(hw), reps=args.reps, warmup=args.warmup,
               note="captured graphs replayed in turn, median ms per call; the yardstick is the same run's plain forecast", runs=[])
    core, st = _fan_setup(B, K, N, hw)
    for Fn in (1, 10, 30):
        variants = [("plain", 1, False), ("fan", S, False)] + ([("fan_lane", S, True)] if args.lane else [])
        g = _fan_graphs(core, st, B, K, N, hw, Fn, variants)
        with core.on_stream():
            ms = _alternate(g, args.reps, args.warmup, core.stream)
        res["runs"].append(dict(B=B, K=K, S=S, F=Fn, ms_per_call=ms, graph_nodes={n: g[n][1] for n in g},
                                lane_ms=ms.get("fan_lane", float("nan")) - ms["fan"]))
        del g
    st.close()
    core, st = _fan_setup(1, 1, N, hw)
    for Fn in (1, 10, 30):
        variants = [("plain", 1, False), ("fan", 32, False)] + ([("fan_lane", 32, True)] if args.lane else [])
        g = _fan_graphs(core, st, 1, 1, N, hw, Fn, variants)
        with core.on_stream():
            ms = _alternate(g, args.reps, args.warmup, core.stream)
        res["runs"].append(dict(B=1, K=1, S=32, F=Fn, ms_per_call=ms, graph_nodes={n: g[n][1] for n in g},
                                lane_ms=ms.get("fan_lane", float("nan")) - ms["fan"]))
        del g
    st.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--samples", type=int, default=None, help="time sqair_forecast_fan with this many rollouts per particle")
    ap.add_argument("--lane", action="store_true", help="with --samples: also the fan with the lane outputs")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if args.lane and args.samples is None:
        ap.error("--lane needs --samples")
    if args.samples is not None:
        return fan_main(args)
    ov, _, _, _ = config_inputs(2)
    B, K, N, hw = 32, int(ov["k_particles"]), int(ov["n_steps_per_image"]), (50, 50)
    F = make_flags(k_particles=K, n_steps_per_image=N)
    obs = torch.as_tensor(to_float(make_sequences(B, T=50, canvas=hw, seed=7)["imgs"])).cuda()
    P = {k: np.asarray(v, dtype=np.float32) for k, v in
         init_params(F, hw, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    core = SqairCore(F, hw)
    core.set_params(P)
    st = SqairStream(core, B, frames_per_step=1, use_graph=True, resample="systematic", ess_frac=0.5)
    frame = [0]

    def step():
        st.step(obs[frame[0] % 50:frame[0] % 50 + 1])
        frame[0] += 1
    with core.on_stream():
        step_ms = _time(step, args.reps, args.warmup, core.stream)
    lib, R, ss = core.lib, B * K, core._stream()
    res = dict(build_id=_capi.build_id(), device=torch.cuda.get_device_name(0), B=B, K=K, N=N, hw=list(hw),
               reps=args.reps, warmup=args.warmup, stream_step_ms_median=float(np.median(step_ms)), forecasts=[])
    for Fn in (1, 10, 30):
        z = lambda *shp: torch.zeros(shp, dtype=torch.float32, device=core.device)
        out = dict(what=z(Fn, R, N, core.nw), where=z(Fn, R, N, 4), presence=z(Fn, R, N), presence_prob=z(Fn, R, N),
                   presence_logit=z(Fn, R, N), obj_id=z(Fn, R, N), canvas=z(Fn, R, *hw), glimpse=z(Fn, R, N, core.G, core.G),
                   mean_canvas=z(Fn, B, *hw), expected_count=z(Fn, B))
        c_out = _capi.SqairForecastOutputs(**{k: v.data_ptr() for k, v in out.items()})
        c_out.log_w = st.log_weight_sum.data_ptr()
        ws = z(lib.sqair_forecast_workspace_bytes(core.handle, Fn, B) // 4)
        noise = z(Fn, R, 2, N, core.nzw)
        core.check(lib.sqair_fill_noise(core.handle, noise.data_ptr(), Fn, B, B, 0, 1, 1 << 63, ss), "sqair_fill_noise")
        a = (core.handle, core.flat.data_ptr(), core.packed.data_ptr(), noise.data_ptr(), Fn, B, st._src.data_ptr(), C.byref(c_out),
             ws.data_ptr(), ws.numel() * 4, ss)
        eager = lambda: core.check(lib.sqair_forecast(*a), "sqair_forecast")
        e_ms = _time(eager, args.reps, args.warmup, core.stream)
        core.stream.synchronize()
        core.check(lib.sqair_capture_begin(core.handle, ss), "sqair_capture_begin")
        core.check(lib.sqair_forecast(*a), "sqair_forecast")
        nodes = lib.sqair_capture_end(core.handle, ss, 0)
        assert nodes > 0, nodes
        g_ms = _time(lambda: core.check(lib.sqair_capture_launch(core.handle, 0, ss), "sqair_capture_launch"), args.reps,
                     args.warmup, core.stream)
        with core.on_stream():
            s_ms = _time(lambda: st.forecast(Fn), args.reps, args.warmup, core.stream)
        res["forecasts"].append(dict(
            F=Fn, graph_nodes=nodes,
            eager_ms_per_call=float(np.median(e_ms)), graph_ms_per_call=float(np.median(g_ms)),
            stream_forecast_ms_per_call=float(np.median(s_ms)),
            eager_us_per_frame=float(np.median(e_ms)) * 1e3 / Fn, graph_us_per_frame=float(np.median(g_ms)) * 1e3 / Fn,
            stream_forecast_us_per_frame=float(np.median(s_ms)) * 1e3 / Fn))
    st.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
