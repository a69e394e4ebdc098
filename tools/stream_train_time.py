#!/usr/bin/env python
"""Step time of training on a stream (sqair_amd.train.StreamTrainer: a carried chunk, include/sqair_hip.h SqairCarry) next to the
plain Trainer.step of the same shape, both graph-replayed, in the same process.  cfg-2's batch (B = 32 sequences x K = 5
particles, N = 4, 50 x 50), T' = 1, 5 and 10 frames per step, the carried step with SMC at chunk boundaries off and on.  A step is
the whole training step of either class: frame copy, Philox noise, the captured forward + ELBO + backward, the optimiser.  HIP
events around every step, each step waiting for the previous one, after a warm-up.

    python tools/stream_train_time.py [--steps 50] [--warmup 10] [--out profiles/stream_train_time.json]

--missing: the cost of a per-frame observed mask in a carried chunk (StreamTrainer(missing=True), the masked pair of calls) at cfg-2's
batch and T' = 10.  Legs alternated round by round in one process: the carried step, the masked step with every lane observed, the
masked step with no lane observed, and the carried step with SMC, whose one extra node prices a node in this very run (the
yardstick of DESIGN.md 3e / 3f).  Reports the masked step's extra time as a multiple of (its extra nodes x that price).

    python tools/stream_train_time.py --missing [--steps 60] [--warmup 10] [--rounds 6] [--out profiles/stream_train_missing_time.json]
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
from sqair_amd.model import Model, SqairCore  # noqa: E402
from sqair_amd.params import init_params  # noqa: E402
from sqair_amd.train import StreamTrainer, Trainer  # noqa: E402


def _timed(step, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for i in range(n):
        ev[i][0].record()
        step(i)
        ev[i][1].record()
        torch.cuda.synchronize()
    ms = np.array([a.elapsed_time(b) for a, b in ev])
    return dict(ms_median=float(np.median(ms)), ms_p10=float(np.percentile(ms, 10)), ms_p90=float(np.percentile(ms, 90)))


def time_shape(T, steps, warmup, B=32, K=5, N=4, hw=(50, 50)):
    F = make_flags(k_particles=K, n_steps_per_image=N, learning_rate=1e-5)
    obs = torch.as_tensor(to_float(make_sequences(B, T=50, canvas=hw, seed=7)["imgs"])).cuda()
    P = {k: np.asarray(v, dtype=np.float32) for k, v in
         init_params(F, hw, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    chunk = lambda i: obs[(i * T) % (50 - T):(i * T) % (50 - T) + T]
    res = dict(T=T, B=B, K=K, N=N, hw=list(hw), steps=steps, warmup=warmup)
    core = SqairCore(F, hw)
    core.set_params(P)
    tr = Trainer(Model(chunk(0), None, core, K, outputs="minimal"), F, collective=False)
    with core.on_stream():
        for i in range(warmup):
            tr.step(chunk(i), seed=1)
        torch.cuda.synchronize()
        res["plain"] = dict(graph_nodes=core.train_graph_nodes, **_timed(lambda i: tr.step(chunk(i), seed=1), steps))
    for smc in (False, True):
        core = SqairCore(F, hw)
        core.set_params(P)
        st = StreamTrainer(core, F, B, frames_per_step=T, collective=False, resample="systematic" if smc else None, outputs=())
        with core.on_stream():
            for i in range(warmup):
                st.step(chunk(i))
            torch.cuda.synchronize()
            res["carry_smc" if smc else "carry"] = dict(graph_nodes=core.train_graph_nodes,
                                                        **_timed(lambda i: st.step(chunk(i)), steps))
    for k in ("carry", "carry_smc"):
        res[k]["overhead_vs_plain"] = res[k]["ms_median"] / res["plain"]["ms_median"] - 1.0
    return res


def time_missing(steps, warmup, rounds, T=10, B=32, K=5, N=4, hw=(50, 50)):
    F = make_flags(k_particles=K, n_steps_per_image=N, learning_rate=1e-5)
    obs = torch.as_tensor(to_float(make_sequences(B, T=50, canvas=hw, seed=7)["imgs"])).cuda()
    P = {k: np.asarray(v, dtype=np.float32) for k, v in
         init_params(F, hw, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    chunk = lambda i: obs[(i * T) % (50 - T):(i * T) % (50 - T) + T]
    every, none = torch.ones(T, B, dtype=torch.bool, device="cuda"), torch.zeros(T, B, dtype=torch.bool, device="cuda")
    # leg: (StreamTrainer arguments, step arguments)
    legs = dict(carry=(dict(), dict()), carry_smc=(dict(resample="systematic"), dict()),
                masked_all_observed=(dict(missing=True), dict(observed=every)),
                masked_none_observed=(dict(missing=True), dict(observed=none)))
    made, ms = {}, {k: [] for k in legs}
    for name, (kw, skw) in legs.items():
        core = SqairCore(F, hw)
        core.set_params(P)
        st = StreamTrainer(core, F, B, frames_per_step=T, collective=False, outputs=(), **kw)
        with core.on_stream():
            for i in range(warmup):
                st.step(chunk(i), **skw)
            torch.cuda.synchronize()
        made[name] = (core, st, skw)
    per_round = max(5, steps // rounds)
    for r in range(rounds):
        for name, (core, st, skw) in made.items():
            with core.on_stream():
                ms[name].append(_timed(lambda i: st.step(chunk(r * per_round + i), **skw), per_round)["ms_median"])
    res = dict(T=T, B=B, K=K, N=N, hw=list(hw), rounds=rounds, steps_per_round=per_round, warmup=warmup)
    for name in legs:
        res[name] = dict(graph_nodes=made[name][0].train_graph_nodes, ms_per_round=ms[name], ms_median=float(np.median(ms[name])))
    node_ms = (res["carry_smc"]["ms_median"] - res["carry"]["ms_median"]) / (res["carry_smc"]["graph_nodes"] - res["carry"]["graph_nodes"])
    res["node_price_ms"] = node_ms
    for name in ("masked_all_observed", "masked_none_observed"):
        extra = res[name]["graph_nodes"] - res["carry"]["graph_nodes"]
        d = res[name]["ms_median"] - res["carry"]["ms_median"]
        res[name].update(extra_nodes=extra, extra_ms=d, multiple_of_node_budget=d / (extra * node_ms) if node_ms > 0 else None)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--missing", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    if args.missing:
        r = time_missing(args.steps, args.warmup, args.rounds)
        for k in ("carry", "carry_smc", "masked_all_observed", "masked_none_observed"):
            print("{:22s} {:.3f} ms ({} nodes)".format(k, r[k]["ms_median"], r[k]["graph_nodes"]), flush=True)
        print("node price {:.4f} ms; masked, every lane observed: +{:.3f} ms = {} x its node budget".format(
            r["node_price_ms"], r["masked_all_observed"]["extra_ms"], r["masked_all_observed"]["multiple_of_node_budget"]))
        out = dict(tool="tools/stream_train_time.py --missing", build_id=_capi.build_id(), device=torch.cuda.get_device_name(0), **r)
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1)
        print(json.dumps(out))
        return
    rows = []
    for T in (1, 5, 10):
        r = time_shape(T, args.steps, args.warmup)
        print("T'={T:2d}  plain {p:.3f} ms ({pn} nodes)  carry {c:.3f} ms ({cn}, {co:+.2%})  carry+SMC {s:.3f} ms ({sn}, {so:+.2%})".format(
            T=T, p=r["plain"]["ms_median"], pn=r["plain"]["graph_nodes"], c=r["carry"]["ms_median"], cn=r["carry"]["graph_nodes"],
            co=r["carry"]["overhead_vs_plain"], s=r["carry_smc"]["ms_median"], sn=r["carry_smc"]["graph_nodes"],
            so=r["carry_smc"]["overhead_vs_plain"]), flush=True)
        rows.append(r)
    out = dict(tool="tools/stream_train_time.py", build_id=_capi.build_id(), device=torch.cuda.get_device_name(0),
               shapes=rows)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
