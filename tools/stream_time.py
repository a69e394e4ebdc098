#!/usr/bin/env python
"""Per-frame latency of streaming inference (sqair_amd/stream.py): SqairStream.step() of ONE frame, graph-replayed (the state
carried in place, default noise from the library's generator), timed with HIP events around every step after a warm-up.

Two shapes: cfg-2's batch (B = 32 sequences x K = 5 particles, N = 4) and one camera (B = 1, K = 1).  The frames are resident on
the device beforehand, so a step is: frame copy, noise fill, the one-frame pass, the output copies and the log-weight sum.

    python tools/stream_time.py [--steps 500] [--warmup 50] [--out profiles/stream_time.json]

With --smc: the same step with in-graph SMC resampling (SqairStream(resample="systematic"), include/sqair_hip.h: sqair_set_smc)
at ess_frac 0.5 and 1.0 next to SMC off, at cfg-2's batch and for one camera with K = 5 particles:

    python tools/stream_time.py --smc [--out profiles/stream_time_smc.json]
"""
import argparse
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


def time_stream(B, K, N, steps, warmup, hw=(50, 50), resample=None, ess_frac=0.5):
    F = make_flags(k_particles=K, n_steps_per_image=N)
    d = make_sequences(B, T=50, canvas=hw, seed=7)   # (fed cyclically)
    obs = torch.as_tensor(to_float(d["imgs"])).cuda()
    P = {k: np.asarray(v, dtype=np.float32) for k, v in
         init_params(F, hw, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    core = SqairCore(F, hw)
    core.set_params(P)
    st = SqairStream(core, B, frames_per_step=1, use_graph=True, resample=resample, ess_frac=ess_frac)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    with core.on_stream():
        for t in range(warmup):
            st.step(obs[t % 50:t % 50 + 1])
        torch.cuda.synchronize()
        for i in range(steps):
            ev[i][0].record()
            st.step(obs[i % 50:i % 50 + 1])
            ev[i][1].record()
            core.stream.synchronize()   # (latency: every step waits for the previous one's results)
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    # back to back: steps issued without waiting, one pair of events around all of them (throughput of a live feed)
    with core.on_stream():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(steps):
            st.step(obs[i % 50:i % 50 + 1])
        b.record()
        torch.cuda.synchronize()
    extra = {}
    if resample is not None:   # (how often the lanes of the last back-to-back step resampled: the work is the same either way)
        extra = dict(resample=resample, ess_frac=ess_frac, resampled_last_step=int(st.resampled.sum()))
    st.close()
    return dict(B=B, K=K, N=N, hw=list(hw), steps=steps, warmup=warmup, graph_nodes=core.graph_nodes(), **extra,
                ms_per_frame_median=float(np.median(ms)), ms_per_frame_p10=float(np.percentile(ms, 10)),
                ms_per_frame_p90=float(np.percentile(ms, 90)), ms_per_frame_back_to_back=float(a.elapsed_time(b) / steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--smc", action="store_true", help="SMC resampling off / ess_frac 0.5 / 1.0 (profiles/stream_time_smc.json)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ov, _, _, _ = config_inputs(2)
    if args.smc:
        shapes = []
        for name, B, K in (("cfg2_batch", 32, ov["k_particles"]), ("one_camera_k5", 1, 5)):
            for resample, frac in ((None, 0.5), ("systematic", 0.5), ("systematic", 1.0)):
                tag = "off" if resample is None else "smc_{}".format(frac)
                shapes.append(dict(name=name + "_" + tag, **time_stream(B, K, ov["n_steps_per_image"], args.steps, args.warmup,
                                                                         resample=resample, ess_frac=frac)))
    else:
        shapes = [dict(name="cfg2_batch", **time_stream(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup)),
                  dict(name="one_camera", **time_stream(1, 1, ov["n_steps_per_image"], args.steps, args.warmup))]
    res = dict(build_id=_capi.build_id(), device=torch.cuda.get_device_name(0), shapes=shapes)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(res, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
