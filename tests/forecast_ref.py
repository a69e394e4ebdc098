"""fp64 reference of the forecast (include/sqair_hip.h: sqair_forecast), composed of the oracle's own pieces: the propagation prior
rolled F frames forward from a carried state, discovery empty -- the reference's generated frame (seq.py:198-200,
sqair_modules.py:157-170, :294-302) -- then the merge and the decoder.

    ref = forecast_ref(orc, state, noise)   # state: SqairOracle.sequence(..., return_state=True)[1], initial_state or gather_state
"""
import numpy as np
import torch

from oracle import sqair_oracle as O

NAMES = ("what", "where", "presence", "presence_prob", "presence_logit", "obj_id", "canvas", "glimpse")
# extras: the prior's statistics of every slot BEFORE the merge (the decisions' margins; which latent regime the rollout visits)
EXTRAS = ("_prior_presence_prob", "_prior_where_scale", "_prior_what_scale", "_prior_logit", "_prior_prev_presence")


def forecast_ref(orc, state, noise):
    """noise [F, B', 2, N, 4 + n_what + 1] (slot s = 0 read).  Returns {name: [F, B', ...] float64} for NAMES, plus
    ``_prior_presence_prob`` [F, B', N] (sigmoid of the prior logit of every slot before the merge: the decisions' margins) and the
    per-frame final state."""
    c = orc.cfg
    N, nw, dt = c.N, c.n_what, orc.dtype
    noise = torch.as_tensor(np.asarray(noise), dtype=dt)
    z, prior, prev_ids, last_id = state.z, state.prior, state.prev_ids, state.last_id
    outs = {n: [] for n in NAMES + EXTRAS}
    with torch.no_grad():
        for f in range(noise.shape[0]):
            eps = noise[f][:, 0]                                      # [B', N, nzw]
            z_prev = z
            (where_loc, where_scale, what_loc, what_scale, logit), prior_new = orc.propagate_prior(z, prior)
            what = what_loc + what_scale * eps[..., 4:4 + nw]
            where = where_loc + where_scale * eps[..., 0:4]
            prob = torch.sigmoid(logit)
            pres = (eps[..., 4 + nw:] < prob).to(dt)                  # [B', N, 1]
            B = what.shape[0]
            none = torch.zeros(B, N, 1, dtype=dt)
            last_id, ids = O.compute_object_ids(last_id, prev_ids, pres, none)   # (discovery contributes nothing)
            prop = [what, where, pres, logit, prob, ids[:, :N], prior_new]
            disc = [torch.zeros_like(x) for x in prop[:5]] + [ids[:, N:], torch.zeros_like(prior_new)]
            widths = [x.shape[-1] for x in prop]
            merged = O.select_present(torch.cat([torch.cat(prop, -1), torch.cat(disc, -1)], 1),
                                      torch.cat([pres, none], 1).squeeze(-1))[:, :N]
            what, where, pres, logit, prob, ids, prior = torch.split(merged, widths, -1)
            canvas, _, glimpse = orc.decode(what, where, pres)
            z, prev_ids = (what, where, pres, logit), ids
            for n, v in zip(NAMES, (what, where, pres, prob, logit, ids, canvas, glimpse)):
                outs[n].append(v.squeeze(-1) if n in ("presence", "presence_prob", "presence_logit", "obj_id") else v)
            outs["_prior_presence_prob"].append(torch.sigmoid(prop[3]).squeeze(-1))
            for n, v in zip(EXTRAS[1:], (where_scale, what_scale, prop[3], z_prev[2])):
                outs[n].append(v)
    res = {n: torch.stack(v, 0) for n, v in outs.items()}
    res["_final"] = (z, prior, prev_ids, last_id)
    return res


def prior_margin(ref, noise):
    """Per row: min over every slot and frame of |u - sigmoid(prior logit)| (the forecast's presence decisions)."""
    u = np.asarray(noise)[:, :, 0, :, -1]
    return np.abs(u - ref["_prior_presence_prob"].numpy()).min((0, 2))
