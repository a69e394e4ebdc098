#!/usr/bin/env python
"""Per-kernel breakdown of a forecast frame (include/sqair_hip.h: sqair_forecast) at cfg-2's batch (B = 32, K = 5, N = 4, 50 x 50).

Workload (run under the profiler): one stream, three eager steps, then 60 synchronous sqair_forecast calls of F = 10:

    rocprofv3 --kernel-trace --output-format csv -d /tmp/fc_trace -- python tools/forecast_trace.py

Reduction of the trace (the first 10 calls are warm-up): median duration of each of the four launches of a forecast frame, the
frame loop's time per frame and the sum of its four kernels' durations, and the launches after the loop -> profiles/forecast_kernel_breakdown.json:

    python tools/forecast_trace.py --analyse /tmp/fc_trace [--out profiles/forecast_kernel_breakdown.json]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload():
    import torch
    from sqair_amd import _capi
    from sqair_amd.data import make_sequences, to_float
    from sqair_amd.flags import make_flags
    from sqair_amd.model import SqairCore
    from sqair_amd.params import init_params
    from sqair_amd.stream import SqairStream
    B, K, N, hw, Fn = 32, 5, 4, (50, 50), 10
    F = make_flags(k_particles=K, n_steps_per_image=N)
    obs = torch.as_tensor(to_float(make_sequences(B, T=3, canvas=hw, seed=7)["imgs"])).cuda()
    P = {k: np.asarray(v, dtype=np.float32) for k, v in init_params(F, hw, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    core = SqairCore(F, hw)
    core.set_params(P)
    st = SqairStream(core, B, frames_per_step=1, use_graph=False, resample="systematic")
    for t in range(3):
        st.step(obs[t:t + 1])
    torch.cuda.synchronize()
    R, lib, ss = B * K, core.lib, core._stream()
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=core.device)
    out = dict(what=z(Fn, R, N, core.nw), where=z(Fn, R, N, 4), presence=z(Fn, R, N), obj_id=z(Fn, R, N), canvas=z(Fn, R, *hw),
               mean_canvas=z(Fn, B, *hw), expected_count=z(Fn, B))
    c_out = _capi.SqairForecastOutputs(**{k: v.data_ptr() for k, v in out.items()})
    c_out.log_w = st.log_weight_sum.data_ptr()
    ws = z(lib.sqair_forecast_workspace_bytes(core.handle, Fn, B) // 4)
    noise = z(Fn, R, 2, N, core.nzw)
    core.check(lib.sqair_fill_noise(core.handle, noise.data_ptr(), Fn, B, B, 0, 1, 1 << 63, ss), "sqair_fill_noise")
    for i in range(60):
        core.check(lib.sqair_forecast(core.handle, core.flat.data_ptr(), core.packed.data_ptr(), noise.data_ptr(), Fn, B, st._src.data_ptr(),
                                      C.byref(c_out), ws.data_ptr(), ws.numel() * 4, ss), "sqair_forecast")
        core.stream.synchronize()
    print("present per frame", out["presence"].sum((1, 2)).tolist())


def analyse(trace_dir, out):
    f = glob.glob(trace_dir + "/**/*kernel_trace.csv", recursive=True)[0]
    ev = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].replace("void ", "").split("(")[0])
                for r in csv.DictReader(open(f)))
    starts = [i for i, e in enumerate(ev) if e[2].startswith("k_init_state")]
    Fn, segs = 10, []
    for a, b in zip(starts, starts[1:] + [len(ev)]):
        names = [e[2] for e in ev[a:b]]
        if any(n.startswith("k_forecast_step") for n in names):
            segs.append(ev[a:b])
    segs = segs[10:]   # (warm-up calls out)
    n_per = [len(s) for s in segs]
    loop = []   # per frame: 4 dispatches (GRU1, GRU2, prior linear, k_forecast_step)
    pos = {}
    for s in segs:
        fr = s[2:2 + 4 * Fn]
        loop.append((fr[-1][1] - s[1][1]) / Fn)
        for j, e in enumerate(fr):
            k = j % 4
            pos.setdefault(k, dict(name=e[2][:60], dur=[]))
            pos[k]["dur"].append(e[1] - e[0])
    tail = {}
    for s in segs:
        for j, e in enumerate(s[2 + 4 * Fn:]):
            tail.setdefault(e[2][:60], []).append(e[1] - e[0])
    res = dict(calls=len(segs), dispatches_per_call=sorted(set(n_per)), frame_loop_us_per_frame=float(np.median(loop)) / 1e3,
               per_frame_kernels=[dict(name=v["name"], kernel_us=float(np.median(v["dur"])) / 1e3)
                                  for k, v in sorted(pos.items())],
               after_loop=[dict(name=k, kernel_us=float(np.median(v)) / 1e3) for k, v in tail.items()])
    # (the frame loop's time not covered by its four kernels: between one dispatch's end and the next one's start)
    res["per_frame_kernels_sum_us"] = sum(k["kernel_us"] for k in res["per_frame_kernels"])
    print(json.dumps(res, indent=1))
    if out:
        json.dump(res, open(out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--analyse", default=None, help="rocprofv3 output directory of a run of this script")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.analyse:
        analyse(args.analyse, args.out)
    else:
        workload()


if __name__ == "__main__":
    main()
