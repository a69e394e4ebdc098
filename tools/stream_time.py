#!/usr/bin/env python
"""Per-frame latency of streaming inference (sqair_amd/stream.py): SqairStream.step() of ONE frame, graph-replayed (the state
carried in place, default noise from the library's generator), timed with HIP events around every step after a warm-up.

Two shapes: cfg-2's batch (B = 32 sequences x K = 5 particles, N = 4) and one camera (B = 1, K = 1).  The frames are resident on
the device beforehand, so a step is: frame copy, noise fill, the one-frame pass, the output copies and the log-weight sum.

    python tools/stream_time.py [--steps 500] [--warmup 50] [--out profiles/stream_time.json]

With --smc: the same step with in-graph SMC resampling (SqairStream(resample="systematic"), include/sqair_hip.h: sqair_set_smc)
at ess_frac 0.5 and 1.0 next to SMC off, at cfg-2's batch and for one camera with K = 5 particles:

    python tools/stream_time.py --smc [--out profiles/stream_time_smc.json]

With --history: the price of the track history (SqairStream(history=64), include/sqair_hip.h: sqair_set_history).  Four streams at
cfg-2's batch in ONE process -- plain, SMC, history, SMC + history --, timed in alternating blocks so that all four see the same
machine, the same minutes.  The yardstick is the same run's SMC on - SMC off difference: the measured price of one dependent graph
node; the push is one node too.  Also the time of tracks() at lag 10 and lag 64, and the ring's bytes:

    python tools/stream_time.py --history [--out profiles/stream_history_time.json]

With --history --lane: the price of the lane tracks (SqairStream.tracks(lag, lane=True), include/sqair_hip.h:
sqair_history_trace_lane) against the plain tracks(lag) of the same run, lag 10 and 64 at cfg-2's batch, alternating in one process.

    python tools/stream_time.py --history --lane [--out profiles/track_lane_time.json]

With --missing: the price of missing-frame steps (SqairStream(missing=True), include/sqair_hip.h: sqair_set_observed).  Streams at
cfg-2's batch alternating in one process as with --history: plain, ``missing=True`` with every lane observed, ``missing=True`` with
no lane observed -- and SMC on, for the yardstick: the same run's SMC on - SMC off difference is the price of one dependent node
that day, and a one-frame pass with a mask has two nodes more.  The ratio is recorded, not gated on:

    python tools/stream_time.py --missing [--out profiles/stream_missing_time.json]

With --estimate: the price of the lane estimate (SqairStream(estimate=True), include/sqair_hip.h: sqair_set_estimate).  Streams at
cfg-2's batch alternating in one process as with --history: plain, SMC, estimate, SMC + estimate, estimate with the posterior mean
reconstruction.  The estimate is one dependent node; the yardstick is the same run's SMC on - SMC off difference, the resampler's
node that day.  The ratio is recorded, not gated on:

    python tools/stream_time.py --estimate [--out profiles/stream_estimate_time.json]

With --layers: the price of the object layers (SqairStream(estimate=True, estimate_layers=True), include/sqair_hip.h:
sqair_set_layers).  Streams at cfg-2's batch alternating in one process as with --history: plain, SMC, estimate, SMC + estimate,
layers, SMC + layers.  The layers are one dependent node after the estimate's -- and a larger copy out of the step: layer and cover
are 2 N H W floats per lane; next to them the estimate's node and the resampler's node of the same run.  Recorded, not gated on:

    python tools/stream_time.py --layers [--out profiles/stream_layers_time.json]

With --score: the price of stream scoring (SqairStream(estimate=True, score=True), include/sqair_hip.h: sqair_set_score).  Streams at
cfg-2's batch alternating in one process as with --history: plain, SMC, estimate, SMC + estimate, score, SMC + score; the scored legs
are fed a truth that is resident on the device (G = N boxes per lane, all present, every frame valid), as the frames are.  The score
is one dependent node after the estimate's, three small copies of the truth into the stream's buffers and six more small fields in
the step's copy of the per-lane answer; next to it the estimate's node and the resampler's node of the same run.  Recorded, not
gated on:

    python tools/stream_time.py --score [--out profiles/stream_score_time.json]

With --identity: the price of lane identities (SqairStream(estimate=True, identity=True), include/sqair_hip.h: sqair_set_identity).
Streams at cfg-2's batch alternating in one process as with --history: plain, SMC, estimate, identity, SMC + estimate, SMC + identity,
score, score + identity (score_ids="lane"); the scored legs are fed a device-resident truth as with --score.  The identity's node is
reported next to the estimate's and the resampler's node of the same run.

    python tools/stream_time.py --identity [--out profiles/stream_identity_time.json]

With --idf: the price of IDF1 scoring (SqairStream(estimate=True, score=True, score_idf=True, score_idf_ids=32), include/sqair_hip.h:
sqair_set_idf).  Streams at cfg-2's batch alternating in one process as with --history: plain, SMC, estimate, SMC + estimate, score,
SMC + score, score + IDF, SMC + score + IDF; the scored legs are fed a device-resident truth as with --score.  The IDF's node is reported
next to the score's and the resampler's node of the same run, and the median time of ``idf_score()`` -- the solve, its three copies
and the host's pooling -- is measured separately.  Recorded, not gated on:

    python tools/stream_time.py --idf [--out profiles/stream_idf_time.json]

With --match: the price of keep + optimal per-frame matching (SqairStream(score_match="optimal" / identity_match="optimal"),
include/sqair_hip.h: sqair_set_lane_match) -- a wavefront's solve where the greedy mode is one thread's walk, in the same one node.
Streams at cfg-2's batch alternating in one process as with --history, all with SMC and the estimate: SMC, SMC + estimate, score greedy,
score optimal, identity greedy, identity optimal; the scored legs are fed a device-resident truth of overlapping boxes.  The difference
optimal - greedy is reported next to the resampler's node of the same run.  Recorded, not gated on:

    python tools/stream_time.py --match [--out profiles/stream_match_time.json]

With --hota: the price of HOTA scoring (SqairStream(estimate=True, score=True, score_hota=True), include/sqair_hip.h: sqair_set_hota).
Streams at cfg-2's batch alternating in one process as with --history: plain, SMC, SMC + estimate, score, SMC + score, score + HOTA,
SMC + score + HOTA; the scored legs are fed a device-resident truth as with --score, and the timed legs' logs are long enough that
every timed step appends a record (a step that finds its log full does less).  The HOTA node is reported next to the score's and the
resampler's node of the same run; the median time of ``hota_score()`` -- the solve over a full log, its copies and the host's ratios
-- is measured separately at ``score_hota_frames`` 64 and 256.  Recorded, not gated on:

    python tools/stream_time.py --hota [--out profiles/stream_hota_time.json]

With --motion: the price of lane motion (SqairStream(estimate=True, identity=True, motion=True), include/sqair_hip.h: sqair_set_motion)
-- the identity's node in its motion instantiation, no node more.  Streams at cfg-2's batch alternating in one process as with
--history, all with SMC and the estimate: SMC, SMC + estimate, identity, motion, motion with nis, identity optimal, motion optimal.  The
difference motion - identity is reported next to the identity's and the resampler's node of the same run.  Recorded, not gated on:

    python tools/stream_time.py --motion [--out profiles/stream_motion_time.json]

With --tracklog: the price of the track log (SqairStream(estimate=True, identity=True, tracklog=L), include/sqair_hip.h:
sqair_set_tracklog) -- one node directly behind the identity's.  Streams at cfg-2's batch alternating in one process as with --history,
all with SMC and the estimate: SMC, SMC + estimate, identity, identity + log, motion, motion + log, and one with a history ring of the
same length beside the log.  The log's node is reported next to the identity's and the resampler's of the same run; ``track_log()`` at
lag 10 and 64 -- the solve, the copies and what the host forms from them, every call waited for -- against ``tracks(lag)`` of the same
run.  Recorded, not gated on:

    python tools/stream_time.py --tracklog [--out profiles/stream_tracklog_time.json]

With --tracklog-score: the price of track log scoring (SqairStream(..., tracklog=L, tracklog_truth=G), ``track_log(lag, score=True)``,
include/sqair_hip.h: sqair_lane_tracklog_score) at cfg-2's batch (L = 64, C = 16, G = 2).  Two streams alternating in one process as
with --history, SMC + estimate + identity + log without and with the truth ring, the second fed a device-resident truth: the difference
is the per-step cost of the ring's copies (no node is added).  Then ``track_log(lag, score=True)`` against ``track_log(lag)`` on the
same stream, alternating, lag 10 and 64, for both matchings, every call waited for; and the scorer alone at the limits of its
arguments (lag 4096, C 64, G 16) on one lane, where lane 0's greedy walk is long.  Recorded, not gated on:

    python tools/stream_time.py --tracklog-score [--out profiles/tracklog_score_time.json]

With --tracklog-fit: the price of motion calibration (``track_log_fit(lag)``, include/sqair_hip.h: sqair_lane_tracklog_fit) at cfg-2's
batch (L = 64, C = 16, the default 8 x 8 grid): ``track_log_fit(lag)`` with and without ``innov`` against ``track_log(lag)`` on the same
stream, alternating, lag 10 and 64, every call waited for.  With --limits only the kernel alone at the limits of its arguments (lag
4096, C 64, a 16 x 16 grid) on one lane, a run of its own so that it can be given its own time limit; its figures are added to the
file --out names.  Recorded, not gated on:

    python tools/stream_time.py --tracklog-fit [--out profiles/tracklog_fit_time.json]
    python tools/stream_time.py --tracklog-fit --limits [--out profiles/tracklog_fit_time.json]
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
from sqair_amd import lane as lane_mod  # noqa: E402
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


def alternating_streams(legs, B, K, N, steps, warmup, rounds, hw, step_kw=None):
    """One stream per leg (name -> SqairStream keywords) in ONE process, timed in alternating blocks so that all of them see the
    same machine, the same minutes.  step_kw: name -> keywords of every step() of that leg.  Returns (streams, the result's
    common fields, median latency per leg, median back-to-back time per leg), times in ms per frame."""
    F = make_flags(k_particles=K, n_steps_per_image=N)
    obs = torch.as_tensor(to_float(make_sequences(B, T=50, canvas=hw, seed=7)["imgs"])).cuda()
    P = {k: np.asarray(v, dtype=np.float32) for k, v in
         init_params(F, hw, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    step_kw = step_kw or {}
    streams = {}
    for name, kw in legs.items():
        core = SqairCore(F, hw)
        core.set_params(P)
        streams[name] = SqairStream(core, B, frames_per_step=1, use_graph=True, **kw)
    block = max(steps // rounds, 1)
    lat = {n: [] for n in legs}   # ms of one step, the host waiting for each (latency)
    b2b = {n: [] for n in legs}   # ms per step of a block issued without waiting (throughput)
    t = 0
    for rnd in range(-1, rounds):  # (round -1: the warm-up, every stream captures its graph)
        for name, st in streams.items():
            core = st.core
            with core.on_stream():
                n = warmup if rnd < 0 else block
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
                kw = step_kw.get(name, {})
                for i in range(n):
                    ev[i][0].record()
                    st.step(obs[(t + i) % 50:(t + i) % 50 + 1], **kw)
                    ev[i][1].record()
                    core.stream.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(n):
                    st.step(obs[(t + i) % 50:(t + i) % 50 + 1], **kw)
                b.record()
                torch.cuda.synchronize()
            if rnd >= 0:
                lat[name] += [x.elapsed_time(y) for x, y in ev]
                b2b[name].append(a.elapsed_time(b) / n)
        t += block
    med = {n: float(np.median(lat[n])) for n in legs}
    thr = {n: float(np.median(b2b[n])) for n in legs}
    res = dict(B=B, K=K, N=N, hw=list(hw), steps=block * rounds, rounds=rounds, warmup=warmup,
               graph_nodes={n: st.core.graph_nodes() for n, st in streams.items()},
               ms_per_frame_median=med, ms_per_frame_p10={n: float(np.percentile(lat[n], 10)) for n in legs},
               ms_per_frame_p90={n: float(np.percentile(lat[n], 90)) for n in legs}, ms_per_frame_back_to_back=thr)
    return streams, res, med, thr


def time_history(B, K, N, steps, warmup, L=64, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    legs = dict(plain={}, smc=smc, history=dict(history=L), smc_history=dict(history=L, **smc))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw)
    res.update(L=L, ring_bytes=int(streams["history"].carried.ring.numel() * 4), history_fields=list(streams["history"].history_fields))
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        push = [v["history"] - v["plain"], v["smc_history"] - v["smc"]]
        res["us_" + key] = dict(smc_node=1e3 * one_node, history_node_on_plain=1e3 * push[0], history_node_on_smc=1e3 * push[1],
                                history_over_smc_node=[p / one_node if one_node > 0 else None for p in push])
    # tracks(): the trace + the track table + the output copies, the ring full (warm-up + steps > L)
    st = streams["smc_history"]
    res["tracks_ms"] = {}
    for lag in (10, L):
        for start in ("next", "last"):
            with st.core.on_stream():
                for _ in range(5):
                    st.tracks(lag=lag, start=start)
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
                for x, y in ev:
                    x.record()
                    st.tracks(lag=lag, start=start)
                    y.record()
                    st.core.stream.synchronize()
            ms = [x.elapsed_time(y) for x, y in ev]
            res["tracks_ms"]["lag{}_{}".format(lag, start)] = dict(median=float(np.median(ms)), p10=float(np.percentile(ms, 10)),
                                                                   p90=float(np.percentile(ms, 90)))
    for st in streams.values():
        st.close()
    return res


def time_track_lane(B, K, N, warmup, L=64, rounds=10, block=10, hw=(50, 50)):
    """The price of the lane tracks: tracks(lag, lane=True) against plain tracks(lag) (the trace, no table in either), lag 10 and L,
    the ring full.  Two SMC + history streams fed the same frames in ONE process -- a stream keeps one set of tracks() buffers, so
    each leg has its own -- called in alternating blocks, every call waited for (latency)."""
    smc = dict(resample="systematic", ess_frac=0.5, history=L)
    legs = dict(tracks=smc, tracks_lane=dict(smc))
    streams, res, _, _ = alternating_streams(legs, B, K, N, max(L, rounds), warmup, rounds, hw)
    res = dict(B=B, K=K, N=N, hw=list(hw), L=L, rounds=rounds, calls_per_leg=rounds * block, ms={}, lane_minus_plain_us={},
               lane_over_plain={})
    calls = dict(tracks=lambda st, lag: st.tracks(lag=lag, table=False), tracks_lane=lambda st, lag: st.tracks(lag=lag, table=False, lane=True))
    for lag in (10, L):
        ms = {n: [] for n in legs}
        for rnd in range(-1, rounds):   # (round -1: the warm-up, every leg allocates its buffers)
            for name, st in streams.items():
                with st.core.on_stream():
                    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(block)]
                    for x, y in ev:
                        x.record()
                        calls[name](st, lag)
                        y.record()
                        st.core.stream.synchronize()
                if rnd >= 0:
                    ms[name] += [x.elapsed_time(y) for x, y in ev]
        med = {n: float(np.median(v)) for n, v in ms.items()}
        key = "lag{}".format(lag)
        res["ms"][key] = {n: dict(median=med[n], p10=float(np.percentile(v, 10)), p90=float(np.percentile(v, 90))) for n, v in ms.items()}
        res["lane_minus_plain_us"][key] = 1e3 * (med["tracks_lane"] - med["tracks"])
        res["lane_over_plain"][key] = med["tracks_lane"] / med["tracks"]
    for st in streams.values():
        st.close()
    return res


def time_missing(B, K, N, steps, warmup, rounds=10, hw=(50, 50)):
    legs = dict(plain={}, smc=dict(resample="systematic", ess_frac=0.5), missing_all_observed=dict(missing=True),
                missing_none_observed=dict(missing=True))
    # (the masks are resident on the device beforehand, as the frames are)
    step_kw = dict(missing_all_observed=dict(observed=torch.ones(B, dtype=torch.bool).cuda()),
                   missing_none_observed=dict(observed=torch.zeros(B, dtype=torch.bool).cuda()))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw, step_kw)
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = {n: v[n] - v["plain"] for n in ("missing_all_observed", "missing_none_observed")}
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for st in streams.values():
        st.close()
    return res


def time_estimate(B, K, N, steps, warmup, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    legs = dict(plain={}, smc=smc, estimate=dict(estimate=True), smc_estimate=dict(estimate=True, **smc),
                canvas=dict(outputs=("what", "where", "presence", "obj_id", "log_weights_per_timestep", "canvas")),
                estimate_canvas=dict(estimate=True, estimate_canvas=True))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw)
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(estimate_node_on_plain=v["estimate"] - v["plain"], estimate_node_on_smc=v["smc_estimate"] - v["smc"],
                     estimate_canvas_on_canvas=v["estimate_canvas"] - v["canvas"])   # (both legs copy the canvases out)
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for st in streams.values():
        st.close()
    return res


def time_layers(B, K, N, steps, warmup, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    lay = dict(estimate=True, estimate_layers=True)
    legs = dict(plain={}, smc=smc, estimate=dict(estimate=True), smc_estimate=dict(estimate=True, **smc), layers=lay,
                smc_layers=dict(lay, **smc))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw)
    res["lane_bytes_per_step"] = {n: int(streams[n]._est_flat.numel() * 4) for n in ("estimate", "layers")}
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(estimate_node_on_plain=v["estimate"] - v["plain"], estimate_node_on_smc=v["smc_estimate"] - v["smc"],
                     layers_node_on_estimate=v["layers"] - v["estimate"], layers_node_on_smc_estimate=v["smc_layers"] - v["smc_estimate"])
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for st in streams.values():
        st.close()
    return res


def time_score(B, K, N, steps, warmup, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    sc = dict(estimate=True, score=True, score_truth=N)
    legs = dict(plain={}, smc=smc, estimate=dict(estimate=True), smc_estimate=dict(estimate=True, **smc), score=sc, smc_score=dict(sc, **smc))
    rng = np.random.default_rng(3)
    box = np.concatenate([rng.uniform(-5, 35, (1, B, N, 2)), rng.uniform(8, 28, (1, B, N, 2))], -1).astype(np.float32)
    truth = dict(box=torch.as_tensor(box).cuda(), present=torch.ones((1, B, N), dtype=torch.int32).cuda(),
                 valid=torch.ones((1, B), dtype=torch.int32).cuda())
    step_kw = dict(score=dict(truth=truth), smc_score=dict(truth=truth))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw, step_kw)
    res["lane_bytes_per_step"] = {n: int(streams[n]._est_flat.numel() * 4) for n in ("estimate", "score")}
    res["score"] = {n: (v.sum().item() if torch.is_tensor(v) else v) for n, v in streams["smc_score"].score().items()}   # (over the lanes)
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(estimate_node_on_plain=v["estimate"] - v["plain"], estimate_node_on_smc=v["smc_estimate"] - v["smc"],
                     score_node_on_estimate=v["score"] - v["estimate"], score_node_on_smc_estimate=v["smc_score"] - v["smc_estimate"])
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for st in streams.values():
        st.close()
    return res


def time_identity(B, K, N, steps, warmup, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    idt = dict(estimate=True, identity=True)
    sc = dict(estimate=True, score=True, score_truth=N)
    legs = dict(plain={}, smc=smc, estimate=dict(estimate=True), identity=idt, smc_estimate=dict(estimate=True, **smc),
                smc_identity=dict(idt, **smc), score=sc, score_identity=dict(sc, identity=True, score_ids="lane"))
    rng = np.random.default_rng(3)
    box = np.concatenate([rng.uniform(-5, 35, (1, B, N, 2)), rng.uniform(8, 28, (1, B, N, 2))], -1).astype(np.float32)
    truth = dict(box=torch.as_tensor(box).cuda(), present=torch.ones((1, B, N), dtype=torch.int32).cuda(),
                 valid=torch.ones((1, B), dtype=torch.int32).cuda())
    step_kw = dict(score=dict(truth=truth), score_identity=dict(truth=truth))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw, step_kw)
    res["lane_bytes_per_step"] = {n: int(streams[n]._est_flat.numel() * 4) for n in ("estimate", "identity")}
    res["identities"] = {n: (int(v.sum()) if torch.is_tensor(v) and v.dim() == 1 else v) for n, v in streams["smc_identity"].identities().items()
                         if not n.startswith("trk_")}   # (over the lanes)
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(estimate_node_on_plain=v["estimate"] - v["plain"], estimate_node_on_smc=v["smc_estimate"] - v["smc"],
                     identity_node_on_estimate=v["identity"] - v["estimate"], identity_node_on_smc_estimate=v["smc_identity"] - v["smc_estimate"],
                     identity_node_on_score=v["score_identity"] - v["score"])
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for st in streams.values():
        st.close()
    return res


def time_idf(B, K, N, steps, warmup, rounds=10, hw=(50, 50), P=32):
    smc = dict(resample="systematic", ess_frac=0.5)
    sc = dict(estimate=True, score=True, score_truth=N)
    idf = dict(sc, score_idf=True, score_idf_ids=P)
    legs = dict(plain={}, smc=smc, estimate=dict(estimate=True), smc_estimate=dict(estimate=True, **smc), score=sc, smc_score=dict(sc, **smc),
                score_idf=idf, smc_score_idf=dict(idf, **smc))
    rng = np.random.default_rng(3)
    box = np.concatenate([rng.uniform(-5, 35, (1, B, N, 2)), rng.uniform(8, 28, (1, B, N, 2))], -1).astype(np.float32)
    truth = dict(box=torch.as_tensor(box).cuda(), present=torch.ones((1, B, N), dtype=torch.int32).cuda(),
                 valid=torch.ones((1, B), dtype=torch.int32).cuda())
    step_kw = {n: dict(truth=truth) for n in ("score", "smc_score", "score_idf", "smc_score_idf")}
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw, step_kw)
    res["P"] = P
    st = streams["smc_score_idf"]
    with st.core.on_stream():   # idf_score(): the solve, the copies and the pooling, every call waited for
        for _ in range(5):
            st.idf_score()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(100)]
        for x, y in ev:
            x.record()
            got = st.idf_score()
            y.record()
            st.core.stream.synchronize()
    ms = [x.elapsed_time(y) for x, y in ev]
    res["idf_score_ms"] = dict(median=float(np.median(ms)), p10=float(np.percentile(ms, 10)), p90=float(np.percentile(ms, 90)))
    res["idf_score"] = {n: (int(v.sum()) if torch.is_tensor(v) else v) for n, v in got.items() if n != "assign"}   # (over the lanes)
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(estimate_node_on_plain=v["estimate"] - v["plain"], score_node_on_estimate=v["score"] - v["estimate"],
                     score_node_on_smc_estimate=v["smc_score"] - v["smc_estimate"], idf_node_on_score=v["score_idf"] - v["score"],
                     idf_node_on_smc_score=v["smc_score_idf"] - v["smc_score"])
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for st in streams.values():
        st.close()
    return res


def time_hota(B, K, N, steps, warmup, rounds=10, hw=(50, 50), P=32, solve_frames=(64, 256)):
    smc = dict(resample="systematic", ess_frac=0.5)
    sc = dict(estimate=True, score=True, score_truth=N)
    L = _capi.HOTA_MAX_FRAMES
    assert 2 * (warmup + max(steps // rounds, 1) * rounds) <= L, "the timed legs' logs would fill up: fewer --steps"
    hota = dict(sc, score_hota=True, score_hota_ids=P, score_hota_frames=L)
    legs = dict(plain={}, smc=smc, smc_estimate=dict(estimate=True, **smc), score=sc, smc_score=dict(sc, **smc), score_hota=hota,
                smc_score_hota=dict(hota, **smc))
    for n in solve_frames:   # (stepped along untimed until their logs are full, for hota_score() below)
        legs["solve_{}".format(n)] = dict(hota, score_hota_frames=n, **smc)
    rng = np.random.default_rng(3)
    box = np.concatenate([rng.uniform(-5, 35, (1, B, N, 2)), rng.uniform(8, 28, (1, B, N, 2))], -1).astype(np.float32)
    truth = dict(box=torch.as_tensor(box).cuda(), present=torch.ones((1, B, N), dtype=torch.int32).cuda(),
                 valid=torch.ones((1, B), dtype=torch.int32).cuda())
    step_kw = {n: dict(truth=truth) for n in legs if "score" in n or n.startswith("solve_")}
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw, step_kw)
    res["P"], res["L_timed_legs"] = P, L
    res["records_in_use"] = {n: int(st._hota["frames"].min()) for n, st in streams.items() if st.lane.hota}
    for n in solve_frames:   # hota_score(): the solve, the copies and the ratios, every call waited for
        st = streams["solve_{}".format(n)]
        assert int(st._hota["frames"].min()) == n, "the log is not full"
        with st.core.on_stream():
            for _ in range(5):
                st.hota_score()
            torch.cuda.synchronize()
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
            for x, y in ev:
                x.record()
                got = st.hota_score()
                y.record()
                st.core.stream.synchronize()
        ms = [x.elapsed_time(y) for x, y in ev]
        res["hota_score_ms_L{}".format(n)] = dict(median=float(np.median(ms)), p10=float(np.percentile(ms, 10)), p90=float(np.percentile(ms, 90)))
        res["hota_score_L{}".format(n)] = {k: got[k] for k in ("hota", "deta", "assa", "loca", "exact")}
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(score_node_on_smc_estimate=v["smc_score"] - v["smc_estimate"], hota_node_on_score=v["score_hota"] - v["score"],
                     hota_node_on_smc_score=v["smc_score_hota"] - v["smc_score"])
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for n in solve_frames:
        for k in ("ms_per_frame_median", "ms_per_frame_p10", "ms_per_frame_p90", "ms_per_frame_back_to_back"):
            res[k].pop("solve_{}".format(n))      # (most of their steps found the log full: not a step's price)
    for st in streams.values():
        st.close()
    return res


def time_match(B, K, N, steps, warmup, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    est = dict(estimate=True, **smc)
    sc = dict(est, score=True, score_truth=N)
    idt = dict(est, identity=True)
    legs = dict(plain={}, smc=smc, smc_estimate=est, score_greedy=sc, score_optimal=dict(sc, score_match="optimal"), identity_greedy=idt,
                identity_optimal=dict(idt, identity_match="optimal"))
    rng = np.random.default_rng(3)     # a crowd: the truths of a lane overlap each other
    centre = rng.uniform(5, 25, (1, B, 1, 2))
    box = np.concatenate([centre + rng.normal(0.0, 3.0, (1, B, N, 2)), rng.uniform(16, 24, (1, B, N, 2))], -1).astype(np.float32)
    truth = dict(box=torch.as_tensor(box).cuda(), present=torch.ones((1, B, N), dtype=torch.int32).cuda(),
                 valid=torch.ones((1, B), dtype=torch.int32).cuda())
    step_kw = dict(score_greedy=dict(truth=truth), score_optimal=dict(truth=truth))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw, step_kw)
    res["score"] = {m: {n: (v.sum().item() if torch.is_tensor(v) else v) for n, v in streams["score_" + m].score().items()}
                    for m in ("greedy", "optimal")}   # (over the lanes)
    res["identities"] = {m: {n: (int(v.sum()) if torch.is_tensor(v) and v.dim() == 1 else v)
                             for n, v in streams["identity_" + m].identities().items() if not n.startswith("trk_")}
                         for m in ("greedy", "optimal")}
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(score_node_greedy=v["score_greedy"] - v["smc_estimate"], score_node_optimal=v["score_optimal"] - v["smc_estimate"],
                     identity_node_greedy=v["identity_greedy"] - v["smc_estimate"],
                     identity_node_optimal=v["identity_optimal"] - v["smc_estimate"],
                     score_optimal_minus_greedy=v["score_optimal"] - v["score_greedy"],
                     identity_optimal_minus_greedy=v["identity_optimal"] - v["identity_greedy"])
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for st in streams.values():
        st.close()
    return res


def time_motion(B, K, N, steps, warmup, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    est = dict(estimate=True, **smc)
    idt = dict(est, identity=True)
    legs = dict(plain={}, smc=smc, smc_estimate=est, identity=idt, motion=dict(idt, motion=True), motion_nis=dict(idt, motion=True, motion_nis=True),
                identity_optimal=dict(idt, identity_match="optimal"), motion_optimal=dict(idt, identity_match="optimal", motion=True))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw)
    res["lane_bytes_per_step"] = {n: int(streams[n]._est_flat.numel() * 4) for n in ("identity", "motion", "motion_nis")}
    res["identities"] = {m: {n: (int(v.sum()) if torch.is_tensor(v) and v.dim() == 1 else v)
                             for n, v in streams[m].identities().items() if not n.startswith("trk_")} for m in ("identity", "motion")}
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(identity_node=v["identity"] - v["smc_estimate"], motion_node=v["motion"] - v["smc_estimate"],
                     motion_minus_identity=v["motion"] - v["identity"], motion_nis_minus_identity=v["motion_nis"] - v["identity"],
                     motion_optimal_minus_identity_optimal=v["motion_optimal"] - v["identity_optimal"])
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    for st in streams.values():
        st.close()
    return res


def time_tracklog(B, K, N, steps, warmup, L=64, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    est = dict(estimate=True, **smc)
    idt = dict(est, identity=True)
    log = dict(tracklog=L, tracklog_tracks=16)
    legs = dict(plain={}, smc=smc, smc_estimate=est, identity=idt, identity_log=dict(idt, **log), motion=dict(idt, motion=True),
                motion_log=dict(idt, motion=True, **log), motion_log_history=dict(idt, motion=True, history=L, **log))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw)
    res.update(L=L, tracks=16, log_bytes=int(sum(t.numel() * t.element_size() for t in streams["motion_log"]._tracklog.values())))
    for key, v in (("latency", med), ("back_to_back", thr)):
        one_node = v["smc"] - v["plain"]            # the yardstick: one dependent node (the resampler) on this machine, this run
        added = dict(identity_node=v["identity"] - v["smc_estimate"], log_node_on_identity=v["identity_log"] - v["identity"],
                     log_node_on_motion=v["motion_log"] - v["motion"])
        res["us_" + key] = dict(smc_node=1e3 * one_node, **{n: 1e3 * a for n, a in added.items()},
                                **{n + "_over_smc_node": (a / one_node if one_node > 0 else None) for n, a in added.items()})
    # track_log() against tracks(): both rings full (warm-up + steps > L), the same stream, every call waited for
    st = streams["motion_log_history"]
    assert int(st._tracklog["count"].min()) >= L, "the log is not full"
    res["ms"] = {}
    for lag in (10, L):
        for name, call in (("track_log", lambda: st.track_log(lag=lag)), ("tracks", lambda: st.tracks(lag=lag))):
            with st.core.on_stream():
                for _ in range(5):
                    got = call()
                torch.cuda.synchronize()
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(50)]
                for x, y in ev:
                    x.record()
                    call()
                    y.record()
                    st.core.stream.synchronize()
            ms = [x.elapsed_time(y) for x, y in ev]
            res["ms"]["{}_lag{}".format(name, lag)] = dict(median=float(np.median(ms)), p10=float(np.percentile(ms, 10)),
                                                           p90=float(np.percentile(ms, 90)))
            if name == "track_log":
                res["n_tracks_lag{}".format(lag)] = dict(mean=float(got["n_tracks"].float().mean()), max=int(got["n_tracks"].max()))
    for k in ("ms_per_frame_median", "ms_per_frame_p10", "ms_per_frame_p90", "ms_per_frame_back_to_back"):
        res[k].pop("motion_log_history")      # (stepped along for the read-outs: not a leg of the comparison)
    for st in streams.values():
        st.close()
    return res


def _timed_calls(core, calls, rounds=10, block=5):
    """{name: [ms]} of the callables ``calls`` in alternating blocks in this process, every call waited for; round -1 is the warm-up."""
    ms = {n: [] for n in calls}
    for rnd in range(-1, rounds):
        for name, call in calls.items():
            with core.on_stream():
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(block)]
                for x, y in ev:
                    x.record()
                    call()
                    y.record()
                    core.stream.synchronize()
            if rnd >= 0:
                ms[name] += [x.elapsed_time(y) for x, y in ev]
    return ms


def _spread(ms):
    return dict(median=float(np.median(ms)), p10=float(np.percentile(ms, 10)), p90=float(np.percentile(ms, 90)))


def scorer_at_the_limits(lag=4096, C=64, G=16, reps=3):
    """k_lane_tracklog_score alone on one lane at the limits of its arguments, on a table made by hand: 64 columns in 16 clusters of four
    around 16 truths, every pair of a cluster eligible, a quarter of the (frame, column)s a gap -- the longest walk lane 0's greedy
    scan has.  Milliseconds per launch, every launch waited for, for both matchings."""
    import ctypes as C_
    core = SqairCore(make_flags(k_particles=2, n_steps_per_image=4), (50, 50))   # (a handle for the error text: the scorer reads nothing else of it)
    lib, h = core.lib, core.handle
    rng = np.random.default_rng(5)
    dev = lambda a: torch.as_tensor(a).cuda()
    centre = np.zeros((lag, 1, C, 2), np.float32)
    cluster = np.arange(C) // 4
    centre[..., 0] = 10.0 + 30.0 * (cluster // 4) + rng.normal(0, 0.4, (lag, 1, C))
    centre[..., 1] = 10.0 + 30.0 * (cluster % 4) + rng.normal(0, 0.4, (lag, 1, C))
    kf = np.zeros((lag, 1, C, 2, 5), np.float32)
    kf[..., 0], kf[..., 2], kf[..., 4] = centre, 1.0, 1.0
    tbox = np.zeros((lag, 1, G, 4), np.float32)
    tbox[..., 0], tbox[..., 1], tbox[..., 2:] = 30.0 * (np.arange(G) // 4), 30.0 * (np.arange(G) % 4), 20.0
    table = dict(track_id=dev(np.arange(C, dtype=np.int32)[None]), frame_index=dev(np.arange(lag, dtype=np.int64)[:, None]),
                 state=dev(np.where(rng.uniform(size=(lag, 1, C)) < 0.25, 2, 1).astype(np.int32)),
                 size=dev(np.full((lag, 1, C, 2), 20.0, np.float32)), filt=dev(kf), smooth=dev(kf))
    log = dict(count=dev(np.full(1, lag, np.int64)), log_valid=dev(np.ones((1, lag), np.int32)), log_id=dev(np.zeros(1, np.int32)),
               log_len=dev(np.zeros(1, np.int32)), log_box=dev(np.zeros(1, np.float32)))   # (only count and log_valid are read)
    truth = dict(truth_box=dev(tbox), truth_present=dev(np.ones((lag, 1, G), np.int32)), truth_valid=dev(np.ones((lag, 1), np.int32)))
    out = {k: torch.zeros(s, dtype=getattr(torch, _capi.field_dtype("SqairTrackLogScore", k)), device="cuda")
           for k, s in _capi.tracklog_score_shapes(lag, 1, G).items()}
    c_log = _capi.SqairLaneTrackLog(L=lag, **{k: t.data_ptr() for k, t in log.items()})
    c_tab = _capi.SqairTrackLogOut(**{k: t.data_ptr() for k, t in table.items()})
    c_truth = _capi.SqairTrackLogTruth(G=G, **{k: t.data_ptr() for k, t in truth.items()})
    c_score = _capi.SqairTrackLogScore(iou_min=0.5, **{k: t.data_ptr() for k, t in out.items()})
    res = dict(lag=lag, C=C, G=G, lanes=1)
    for match, name in enumerate(("greedy", "optimal")):
        ms = []
        for i in range(reps + 1):   # (the first launch loads the code object: not counted)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = lib.sqair_lane_tracklog_score(h, C_.byref(c_log), C_.byref(c_tab), C_.byref(c_truth), C_.byref(c_score), lag, C, 1, match,
                                               C_.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, lib.sqair_last_error(h)
            b.record()
            torch.cuda.synchronize()
            if i:
                ms.append(a.elapsed_time(b))
        counts = dict(zip(_capi.TRACKLOG_SCORE_COUNTS, out["counts"][0, 3].tolist()))
        res[name] = dict(ms=_spread(ms), smooth_filled={k: counts[k] for k in ("frames", "truth", "tp", "fn", "fp", "idtp")})
    return res


def time_tracklog_score(B, K, N, steps, warmup, L=64, G=2, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    idt = dict(estimate=True, identity=True, tracklog=L, tracklog_tracks=16, **smc)
    legs = dict(log=idt, log_truth=dict(idt, tracklog_truth=G))
    rng = np.random.default_rng(3)
    box = np.concatenate([rng.uniform(-5, 35, (1, B, G, 2)), rng.uniform(8, 28, (1, B, G, 2))], -1).astype(np.float32)
    truth = dict(box=torch.as_tensor(box).cuda(), present=torch.ones((1, B, G), dtype=torch.int32).cuda(),
                 valid=torch.ones((1, B), dtype=torch.int32).cuda())
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw, dict(log_truth=dict(truth=truth)))
    res.update(L=L, tracks=16, G=G, ring_bytes=int(sum(t.numel() * t.element_size() for t in streams["log_truth"]._truth_ring.values())))
    res["us_ring_copies_per_step"] = dict(latency=1e3 * (med["log_truth"] - med["log"]), back_to_back=1e3 * (thr["log_truth"] - thr["log"]))
    st = streams["log_truth"]
    assert int(st._tracklog["count"].min()) >= L and st.lane.ring_frames >= L, "the log is not full"
    res["ms"], res["score_minus_plain_us"] = {}, {}
    for lag in (10, L):
        calls = dict(track_log=lambda: st.track_log(lag=lag),
                     score_greedy=lambda: st.track_log(lag=lag, score=True, score_match="greedy"),
                     score_optimal=lambda: st.track_log(lag=lag, score=True, score_match="optimal"))
        ms = _timed_calls(st.core, calls)
        key = "lag{}".format(lag)
        res["ms"][key] = {n: _spread(v) for n, v in ms.items()}
        res["score_minus_plain_us"][key] = {n: 1e3 * (float(np.median(ms[n])) - float(np.median(ms["track_log"])))
                                            for n in ("score_greedy", "score_optimal")}
        sc = st.track_log(lag=lag, score=True)["score"]["smooth_filled"]
        res["smooth_filled_" + key] = {n: (int(v.sum()) if torch.is_tensor(v) and v.dim() == 1 and not v.is_floating_point() else v)
                                       for n, v in sc.items() if n in ("frames", "truth", "tp", "fn", "fp", "gap_tp", "gap_fp", "mota", "idf1")}
    for st in streams.values():
        st.close()
    res["scorer_at_the_limits"] = scorer_at_the_limits()
    return res


def fit_at_the_limits(lag=4096, C=64, N=16, Q=16, R=16, reps=3):
    """k_lane_tracklog_fit alone on one lane at the limits of its arguments, on a table made by hand: 64 columns seen in every frame
    but a tenth of them (gaps), 256 candidates -- two a round, eight rounds a workgroup, 128 staged blocks a round, 4096 steps a
    thread.  Milliseconds per launch, every launch waited for."""
    import ctypes as C_
    core = SqairCore(make_flags(k_particles=2, n_steps_per_image=4), (50, 50))   # (a handle for the error text: the fit reads nothing else of it)
    lib, h = core.lib, core.handle
    rng = np.random.default_rng(5)
    dev = lambda a: torch.as_tensor(a).cuda()
    box = np.zeros((1, lag, N, 4), np.float32)
    box[..., :2] = 100.0 + np.cumsum(rng.normal(0, 1.0, (1, lag, N, 2)), 1)
    box[..., 2:] = 10.0
    state = np.where(rng.uniform(size=(lag, 1, C)) < 0.1, 2, 1).astype(np.int32)
    state[0] = 1
    table = dict(frame_index=dev(np.arange(lag, dtype=np.int64)[:, None]), state=dev(state))
    work = dev(np.broadcast_to(np.arange(C, dtype=np.int32) % N, (1, lag, C)).copy())
    log = dict(count=dev(np.full(1, lag, np.int64)), log_valid=dev(np.ones((1, lag), np.int32)), log_id=dev(np.zeros(1, np.int32)),
               log_len=dev(np.zeros(1, np.int32)), log_box=dev(box))   # (only L and log_box are read)
    out = {k: torch.zeros(s, dtype=getattr(torch, _capi.field_dtype("SqairTrackLogFit", k)), device="cuda")
           for k, s in _capi.tracklog_fit_shapes(lag, 1, C, Q, R).items()}
    c_log = _capi.SqairLaneTrackLog(L=lag, **{k: t.data_ptr() for k, t in log.items()})
    c_tab = _capi.SqairTrackLogOut(**{k: t.data_ptr() for k, t in table.items()})
    grid = [0.01 * 2.0 ** k for k in range(16)]
    c_fit = _capi.tracklog_fit_struct(grid[:Q], grid[:R], 16.0, 2, **{k: t.data_ptr() for k, t in out.items()})
    ms = []
    for i in range(reps + 1):   # (the first launch loads the code object: not counted)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = lib.sqair_lane_tracklog_fit(h, C_.byref(c_log), C_.byref(c_tab), work.data_ptr(), C_.byref(c_fit), lag, C, N, 1,
                                         C_.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, lib.sqair_last_error(h)
        b.record()
        torch.cuda.synchronize()
        if i:
            ms.append(a.elapsed_time(b))
    fit = lane_mod.track_log_fit({k: t.cpu() for k, t in out.items() if k != "innov"}, grid[:Q], grid[:R])
    return dict(lag=lag, C=C, N=N, Q=Q, R=R, lanes=1, ms=_spread(ms), terms=int(fit["n"][fit["node"]]), q=fit["q"], r=fit["r"],
                mean_nis=float(fit["mean_nis"][fit["node"]]))


def time_tracklog_fit(B, K, N, steps, warmup, L=64, rounds=10, hw=(50, 50)):
    smc = dict(resample="systematic", ess_frac=0.5)
    legs = dict(log=dict(estimate=True, identity=True, tracklog=L, tracklog_tracks=16, **smc))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw)
    st = streams["log"]
    assert int(st._tracklog["count"].min()) >= L, "the log is not full"
    res.update(L=L, tracks=16, grid=[8, 8], burn=2)
    res["ms"], res["fit_minus_plain_us"] = {}, {}
    for lag in (10, L):
        calls = dict(track_log=lambda: st.track_log(lag=lag), track_log_fit=lambda: st.track_log_fit(lag=lag),
                     track_log_fit_innov=lambda: st.track_log_fit(lag=lag, innov=True))
        ms = _timed_calls(st.core, calls)
        key = "lag{}".format(lag)
        res["ms"][key] = {n: _spread(v) for n, v in ms.items()}
        res["fit_minus_plain_us"][key] = {n: 1e3 * (float(np.median(ms[n])) - float(np.median(ms["track_log"])))
                                          for n in ("track_log_fit", "track_log_fit_innov")}
        fit = st.track_log_fit(lag=lag)
        res["fit_" + key] = dict(node=fit["node"], q=fit["q"], r=fit["r"], at_edge=fit["at_edge"], terms=int(fit["n"].max()),
                                 mean_nis_at_the_fit=float(fit["mean_nis"][fit["node"]]) if fit["node"] else None,
                                 mean_nis_at_the_defaults=float(fit["mean_nis"][4, 4]))
    for st in streams.values():
        st.close()
    return res


def time_tracklog_stitch(B, K, N, steps, warmup, L=64, rounds=10, hw=(50, 50)):
    """track_log(lag, stitch=True) against track_log(lag) on the same stream, alternating, at lag 10 and L."""
    smc = dict(resample="systematic", ess_frac=0.5)
    legs = dict(log=dict(estimate=True, identity=True, tracklog=L, tracklog_tracks=16, **smc))
    streams, res, med, thr = alternating_streams(legs, B, K, N, steps, warmup, rounds, hw)
    st = streams["log"]
    assert int(st._tracklog["count"].min()) >= L, "the log is not full"
    res.update(L=L, tracks=16, gate=3.5)
    res["ms"], res["stitch_minus_plain_us"], res["links"] = {}, {}, {}
    for lag in (10, L):
        calls = dict(track_log=lambda: st.track_log(lag=lag), track_log_stitch=lambda: st.track_log(lag=lag, stitch=True))
        ms = _timed_calls(st.core, calls)
        key = "lag{}".format(lag)
        res["ms"][key] = {n: _spread(v) for n, v in ms.items()}
        res["stitch_minus_plain_us"][key] = 1e3 * (float(np.median(ms["track_log_stitch"])) - float(np.median(ms["track_log"])))
        got = st.track_log(lag=lag, stitch=True)
        res["links"][key] = dict(links=int(got["stitched"]["links"]["n_links"].sum()), tracks=int(got["n_tracks"].sum()),
                                 stitched_tracks=int(got["stitched"]["n_tracks"].sum()))
    for st in streams.values():
        st.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--smc", action="store_true", help="SMC resampling off / ess_frac 0.5 / 1.0 (profiles/stream_time_smc.json)")
    ap.add_argument("--history", action="store_true", help="plain / SMC / history / SMC + history, alternating (profiles/stream_history_time.json)")
    ap.add_argument("--lane", action="store_true", help="with --history: tracks(lag, lane=True) against tracks(lag), alternating (profiles/track_lane_time.json)")
    ap.add_argument("--missing", action="store_true", help="plain / SMC / a mask with every lane / with no lane observed, alternating (profiles/stream_missing_time.json)")
    ap.add_argument("--estimate", action="store_true", help="plain / SMC / estimate / SMC + estimate / with mean_canvas, alternating (profiles/stream_estimate_time.json)")
    ap.add_argument("--layers", action="store_true", help="plain / SMC / estimate / SMC + estimate / layers / SMC + layers, alternating (profiles/stream_layers_time.json)")
    ap.add_argument("--score", action="store_true", help="plain / SMC / estimate / SMC + estimate / score / SMC + score, alternating (profiles/stream_score_time.json)")
    ap.add_argument("--identity", action="store_true", help="plain / SMC / estimate / identity / SMC + estimate / SMC + identity / score / score + identity, alternating (profiles/stream_identity_time.json)")
    ap.add_argument("--idf", action="store_true", help="score and score + IDF, each with and without SMC, alternating; idf_score() apart (profiles/stream_idf_time.json)")
    ap.add_argument("--match", action="store_true", help="score and identity, greedy and optimal, with SMC and the estimate, alternating (profiles/stream_match_time.json)")
    ap.add_argument("--hota", action="store_true", help="score and score + HOTA, each with and without SMC, alternating; hota_score() apart (profiles/stream_hota_time.json)")
    ap.add_argument("--motion", action="store_true", help="identity and identity + motion, greedy and optimal, with SMC and the estimate, alternating (profiles/stream_motion_time.json)")
    ap.add_argument("--tracklog", action="store_true", help="identity and motion with and without the track log, with SMC and the estimate, alternating; track_log() against tracks() apart (profiles/stream_tracklog_time.json)")
    ap.add_argument("--tracklog-score", action="store_true", help="the track log with and without its truth ring, alternating; track_log(score=True) against track_log(); the scorer at its limits (profiles/tracklog_score_time.json)")
    ap.add_argument("--tracklog-fit", action="store_true", help="track_log_fit(lag) against track_log(lag) at lag 10 and 64 with the 8 x 8 grid (profiles/tracklog_fit_time.json); with --limits: k_lane_tracklog_fit alone at its limits, added to the file --out names")
    ap.add_argument("--tracklog-stitch", action="store_true", help="track_log(lag, stitch=True) against track_log(lag) at lag 10 and 64, alternating (profiles/tracklog_stitch_time.json)")
    ap.add_argument("--limits", action="store_true", help="with --tracklog-fit: only the kernel at the limits of its arguments (lag 4096, C 64, 16 x 16, one lane)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    ov, _, _, _ = config_inputs(2)
    if args.tracklog_fit and args.limits:
        res = json.load(open(args.out)) if args.out and os.path.exists(args.out) else dict(build_id=_capi.build_id(), device=torch.cuda.get_device_name(0), shapes=[])
        assert res["build_id"] == _capi.build_id(), "the file was written by another build"
        res["fit_at_the_limits"] = fit_at_the_limits()
        print(json.dumps(res["fit_at_the_limits"]))
        if args.out:
            json.dump(res, open(args.out, "w"), indent=1)
        return
    if args.tracklog_stitch:
        shapes = [dict(name="cfg2_batch_tracklog_stitch", **time_tracklog_stitch(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.tracklog_fit:
        shapes = [dict(name="cfg2_batch_tracklog_fit", **time_tracklog_fit(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.tracklog_score:
        shapes = [dict(name="cfg2_batch_tracklog_score", **time_tracklog_score(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.tracklog:
        shapes = [dict(name="cfg2_batch_tracklog", **time_tracklog(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.motion:
        shapes = [dict(name="cfg2_batch_motion", **time_motion(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.hota:
        shapes = [dict(name="cfg2_batch_hota", **time_hota(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.match:
        shapes = [dict(name="cfg2_batch_match", **time_match(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.idf:
        shapes = [dict(name="cfg2_batch_idf", **time_idf(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.identity:
        shapes = [dict(name="cfg2_batch_identity", **time_identity(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.score:
        shapes = [dict(name="cfg2_batch_score", **time_score(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.layers:
        shapes = [dict(name="cfg2_batch_layers", **time_layers(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.estimate:
        shapes = [dict(name="cfg2_batch_estimate", **time_estimate(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.missing:
        shapes = [dict(name="cfg2_batch_missing", **time_missing(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.history and args.lane:
        shapes = [dict(name="cfg2_batch_track_lane", **time_track_lane(32, ov["k_particles"], ov["n_steps_per_image"], args.warmup))]
    elif args.history:
        shapes = [dict(name="cfg2_batch_history", **time_history(32, ov["k_particles"], ov["n_steps_per_image"], args.steps, args.warmup))]
    elif args.smc:
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
