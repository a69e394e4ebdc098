"""How much keep + optimal per-frame matching (include/sqair_hip.h: sqair_set_lane_match) changes a scored stream on the project's own
data: two streams over the same 100 frames of ``make_sequences(32, T=100, n_objects=(0, 2))`` -- SMC, the estimate, the score against
the data's ``coords`` -- one with ``score_match="greedy"``, one with ``"optimal"``.  Everything the score does not write is the same
in both, so the two see the same lane answer frame by frame; reported: the scored frames, the share of them in which the two differ
(in tp, in the sum of match_iou, in truth_match at all), and both streams' totals and mota.  The result joins
profiles/match_parity.json under "stream":

    python tools/match_parity.py [--out profiles/match_parity.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    B, T, K, N, hw = 32, 100, 5, 4, (50, 50)
    d = make_sequences(B, T=T, canvas=hw, n_objects=(0, 2), seed=7)
    obs = torch.as_tensor(to_float(d["imgs"])).cuda()
    G = d["coords"].shape[2]
    F = make_flags(k_particles=K, n_steps_per_image=N)
    P = {k: np.asarray(v, dtype=np.float32) for k, v in init_params(F, hw, seed=0, mean_img=obs.mean((0, 1)).cpu().numpy(), jitter=0.02).items()}
    streams = {}
    for mode in ("greedy", "optimal"):
        core = SqairCore(F, hw)
        core.set_params(P)
        streams[mode] = SqairStream(core, B, estimate=True, score=True, score_truth=G, score_match=mode, resample="systematic", ess_frac=0.5,
                                    seed=5)
    scored = differ = differ_tp = differ_sum = 0
    for t in range(T):
        truth = dict(box=d["coords"][t:t + 1], present=(d["nums"][t:t + 1, :, :G] != 0).astype(np.int32))
        lanes = {m: {n: v.cpu().numpy() for n, v in st.step(obs[t:t + 1], truth=truth)["lane"].items()} for m, st in streams.items()}
        g, o = lanes["greedy"], lanes["optimal"]
        assert np.array_equal(g["box"].view(np.int32), o["box"].view(np.int32))      # (the same lane answer in both)
        on = g["tp"] >= 0
        scored += int(on.sum())
        differ += int(((g["truth_match"] != o["truth_match"]).any(-1) & on).sum())
        differ_tp += int(((g["tp"] != o["tp"]) & on).sum())
        differ_sum += int(((np.abs(g["match_iou"].astype(np.float64).sum(-1) - o["match_iou"].astype(np.float64).sum(-1)) > 0) & on).sum())
    res = dict(build_id=_capi.build_id(), device=torch.cuda.get_device_name(0), B=B, T=T, K=K, N=N, G=int(G), scored_frames=scored,
               differ=differ / max(scored, 1), differ_tp=differ_tp / max(scored, 1), differ_iou_sum=differ_sum / max(scored, 1))
    for m, st in streams.items():
        res[m] = {n: (v.sum().item() if torch.is_tensor(v) else v) for n, v in st.score().items()}
        st.close()
    print(json.dumps(res))
    if args.out:
        data = json.load(open(args.out)) if os.path.exists(args.out) else {}
        data["stream"] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(data, open(args.out, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
