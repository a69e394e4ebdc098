#!/usr/bin/env python
"""The price of trajectory scoring (SqairStream.forecast / tracks(lane=True, truth=...), include/sqair_hip.h: sqair_lane_traj_score):
at cfg-2's batch (B = 32 sequences x K = 5 particles, N = 4, 50 x 50) ``forecast(10, samples=8, lane=True)`` and ``tracks(10,
lane=True)``, each without ``truth``, with a truth on the host (uploaded by the call) and with a truth already resident on the device
(G = N slots per lane, made from the call's own table).  The six variants alternate in ONE process, block by block, so that all of
them see the same machine, the same minutes; every call is timed with HIP events, the host waiting for each (latency).  The score is
one more launch after the call's own, six small uploads when the truth comes from the host, and seven more small fields copied out.

Next to the figures go the parent's for the same two calls, from profiles/forecast_lane_time.json and profiles/track_lane_time.json --
those time the C-ABI calls as replayed graphs, these the Python calls, so the pair says what a score adds, not what Python costs.
Nothing is gated on: nobody has measured this node before.  ``--bench NAME=FILE`` (repeatable) embeds result lines of bench.py, for
the record of the frame loop's step on this build and on the parent's, measured in the same session.

    python tools/traj_score_time.py [--rounds 10] [--calls 20] [--out profiles/traj_score_time.json] [--bench this=a.json --bench parent=b.json]
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
from sqair_amd.data import make_sequences, to_float  # noqa: E402
from sqair_amd.flags import make_flags  # noqa: E402
from sqair_amd.model import SqairCore  # noqa: E402
from sqair_amd.params import init_params  # noqa: E402
from sqair_amd.stream import SqairStream  # noqa: E402

B, K, N, HW = 32, 5, 4, (50, 50)
F_FORECAST, S, LAG, HISTORY, STEPS = 10, 8, 10, 16, 12


def truth_of(lane, tracks):
    """A truth of G = N slots from a lane table: the table's own boxes (a tracker with random parameters follows nothing else)."""
    living = (lane["alive"] > 0) & (lane["presence"] != 0)[None]
    ones = lambda *shape: torch.ones(shape, dtype=torch.int32, device=living.device)
    t = dict(box=torch.where(living[..., None], lane["box_mean"], torch.zeros_like(lane["box_mean"])), present=living.to(torch.int32),
             valid=ones(*living.shape[:2]))
    if not tracks:
        t.update(anchor_box=lane["box0"].clone(), anchor_present=(lane["presence"] != 0).to(torch.int32), anchor_valid=ones(living.shape[1]))
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20, help="calls per variant and round")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traj_score_time.json"))
    ap.add_argument("--bench", action="append", default=[], metavar="NAME=FILE", help="a file holding a result line of bench.py")
    args = ap.parse_args()
    flags = make_flags(k_particles=K, n_steps_per_image=N)
    obs = torch.as_tensor(to_float(make_sequences(B, T=STEPS, canvas=HW, seed=7)["imgs"])).cuda()
    P = {k: np.asarray(v, dtype=np.float32) for k, v in
         init_params(flags, HW, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    core = SqairCore(flags, HW)
    core.set_params(P)
    st = SqairStream(core, B, frames_per_step=1, use_graph=True, history=HISTORY)
    for t in range(STEPS):
        st.step(obs[t:t + 1])
    calls = dict(forecast=lambda **kw: st.forecast(F_FORECAST, samples=S, lane=True, **kw), tracks=lambda **kw: st.tracks(LAG, lane=True, **kw))
    variants = {}
    for kind, call in calls.items():
        dev = truth_of(call()["lane"], kind == "tracks")
        torch.cuda.synchronize()
        host = {n: v.cpu() for n, v in dev.items()}
        variants[kind] = lambda call=call: call()
        variants[kind + "_truth_host"] = lambda call=call, host=host: call(truth=host)
        variants[kind + "_truth_device"] = lambda call=call, dev=dev: call(truth=dev)
    ms = {n: [] for n in variants}
    for rnd in range(-1, args.rounds):      # (round -1: the warm-up, every variant allocates its buffers)
        for name, fn in variants.items():
            for _ in range(args.calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with core.on_stream():
                    a.record()
                    fn()
                    b.record()
                core.stream.synchronize()
                torch.cuda.synchronize()
                if rnd >= 0:
                    ms[name].append(a.elapsed_time(b))
    stat = lambda v: dict(median=float(np.median(v)), p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90)))
    res = {n: stat(v) for n, v in ms.items()}
    scored = {kind: {n: int(v.sum()) for n, v in st.trajectory_score(kind).items() if n in ("calls", "frames", "pairs", "linked")} for kind in calls}
    parent = {}
    try:
        fl = json.load(open(os.path.join(ROOT, "profiles", "forecast_lane_time.json")))
        run = [r for r in fl["runs"] if (r["B"], r["K"], r["S"], r["F"]) == (B, K, S, F_FORECAST)][0]
        parent["forecast_fan_lane_graph_ms"] = dict(build_id=fl["build_id"], ms=run["ms_per_call"]["fan_lane"])
        tl = json.load(open(os.path.join(ROOT, "profiles", "track_lane_time.json")))
        parent["tracks_lane_lag10_ms"] = dict(build_id=tl["build_id"], ms=tl["shapes"][0]["ms"]["lag10"]["tracks_lane"]["median"])
    except (OSError, KeyError, IndexError):
        pass
    bench = {}
    for item in args.bench:
        name, path = item.split("=", 1)
        lines = [l for l in open(path).read().splitlines() if l.startswith("{")]
        line = json.loads(lines[-1])
        bench.setdefault(name, []).append({k: line.get(k) for k in ("build_id", "ms_per_step", "value", "unit", "steps", "warmup")})
    out = dict(build_id=_capi.build_id(), device=torch.cuda.get_device_name(0), B=B, K=K, N=N, hw=list(HW), G=N, F=F_FORECAST, S=S, lag=LAG,
               history=HISTORY, rounds=args.rounds, calls_per_round=args.calls,
               note="ms per Python call, HIP events, the host waiting for each; the six variants alternate in one process.  parent: the "
                    "same two calls as replayed C-ABI graphs on the parent's builds (another session, another way of calling): beside, "
                    "not against.  Recorded, gated on nothing.",
               ms=res, scored=scored, parent=parent,
               truth_minus_plain_us={kind: {v: 1e3 * (res[kind + "_truth_" + v]["median"] - res[kind]["median"]) for v in ("host", "device")}
                                     for kind in calls})
    if bench:
        out["bench"] = bench
    st.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(dict(ms={n: round(v["median"], 4) for n, v in res.items()}, truth_minus_plain_us=out["truth_minus_plain_us"])))


if __name__ == "__main__":
    main()
