"""fp64 reference of the missing-frame steps (include/sqair_hip.h: sqair_set_observed), one frame at a time over SqairOracle
states.  Observed rows take ``orc.sequence`` for the frame.  Unobserved rows take the prior step, composed of the oracle's own
pieces as tests/forecast_ref.py is -- propagate_prior, compute_object_ids, select_present, decode -- with the HELD temporal state
among the merged features (the reference's merge, select_present over [temporal_prev | init_temporal] with discovery absent:
oracle/sqair_oracle.py, SqairOracle.timestep) and the frame counter advanced.  Rows are chosen by torch.where on the mask.

    out, state = coast_ref(orc, state, tiled_obs, noise, observed)
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import sqair_oracle as O
from tests.hip_util import presence_margins

SLOT_NAMES = ("presence", "presence_prob", "presence_logit", "obj_id")
COASTED = ("what", "where", "presence", "presence_prob", "presence_logit", "obj_id", "canvas", "glimpse")
COUNTS = ("num_prop_steps_per_sample", "num_steps_per_sample", "prop_pres")


def prior_frame(orc, state, eps):
    """One coasted frame of every row.  eps [B', N, nzw]: noise slot s = 0 of the frame.  Returns ({name: value} for COASTED and
    COUNTS plus ``_prior_presence_prob`` [B', N], the state after the frame)."""
    c = orc.cfg
    N, nw, dt = c.N, c.n_what, orc.dtype
    z, prior, temporal, prev_ids, last_id = state.z, state.prior, state.temporal, state.prev_ids, state.last_id
    (where_loc, where_scale, what_loc, what_scale, logit), prior_new = orc.propagate_prior(z, prior)
    what = what_loc + what_scale * eps[..., 4:4 + nw]
    where = where_loc + where_scale * eps[..., 0:4]
    prob = torch.sigmoid(logit)
    pres = (eps[..., 4 + nw:] < prob).to(dt)                  # [B', N, 1]
    B = what.shape[0]
    none = torch.zeros(B, N, 1, dtype=dt)
    last_new, ids = O.compute_object_ids(last_id, prev_ids, pres, none)   # (discovery contributes nothing: last_id stays)
    init_temporal = orc.initial_temporal_state()[None].expand(B, N, -1)
    init_prior = orc.initial_prior_state()[None].expand(B, N, -1)
    prop = [what, where, pres, logit, prob, ids[:, :N], prior_new, temporal]
    disc = [torch.zeros_like(x) for x in prop[:5]] + [ids[:, N:], init_prior, init_temporal]
    widths = [x.shape[-1] for x in prop]
    merged = O.select_present(torch.cat([torch.cat(prop, -1), torch.cat(disc, -1)], 1), torch.cat([pres, none], 1).squeeze(-1))[:, :N]
    what, where, pres_m, logit_m, prob_m, ids_m, prior_m, temporal_m = torch.split(merged, widths, -1)
    canvas, _, glimpse = orc.decode(what, where, pres_m)
    n = pres_m.squeeze(-1).sum(-1)
    out = dict(what=what, where=where, presence=pres_m.squeeze(-1), presence_prob=prob_m.squeeze(-1), presence_logit=logit_m.squeeze(-1),
               obj_id=ids_m.squeeze(-1), canvas=canvas, glimpse=glimpse, num_prop_steps_per_sample=n, num_steps_per_sample=n,
               prop_pres=pres_m.squeeze(-1), _prior_presence_prob=prob.squeeze(-1))
    new = SimpleNamespace(z=(what, where, pres_m, logit_m), temporal=temporal_m, prior=prior_m, prev_ids=ids_m, last_id=last_new,
                          t=state.t + 1)
    return out, new


def _pick(mask, a, b):
    """Rows of ``a`` where mask, of ``b`` elsewhere (mask [B'])."""
    return torch.where(mask.reshape((-1,) + (1,) * (a.dim() - 1)), a, b)


def coast_ref(orc, state, tiled_obs, noise, observed):
    """tiled_obs [T, B', H, W]; noise [T, B', 2, N, nzw]; observed [T, B] bool (B' = B * K rows, K per lane).  Returns
    ({name: [T, B', ...] float64} for every reference output, zeros where the header says so, plus ``presence_margins`` [T, B']
    (the posterior decisions of observed rows; 1 for coasted ones) and ``prior_margin`` [T, B'] (the prior draws of coasted rows; 1
    for observed ones), the state after the T frames)."""
    dt = orc.dtype
    tiled_obs = torch.as_tensor(np.asarray(tiled_obs), dtype=dt)
    noise_np = np.asarray(noise)
    noise = torch.as_tensor(noise_np, dtype=dt)
    observed = np.asarray(observed, dtype=bool)
    T, R = noise.shape[:2]
    K = R // observed.shape[1]
    outs, m_post, m_prior = {}, [], []
    with torch.no_grad():
        for t in range(T):
            rows = torch.as_tensor(np.repeat(observed[t], K))
            img = torch.where(rows[:, None, None], tiled_obs[t], torch.zeros((), dtype=dt))   # (what the stream feeds; never matters)
            so, s_obs = orc.sequence(img[None], noise[t:t + 1], state=state, return_state=True)
            co, s_coast = prior_frame(orc, state, noise[t, :, 0])
            for n, v in so.items():
                if n.startswith("_"):
                    continue
                v = v[0]
                outs.setdefault(n, []).append(_pick(rows, v, co[n] if n in COASTED + COUNTS else torch.zeros_like(v)))
            m_post.append(np.where(rows.numpy(), presence_margins(so, noise_np[t:t + 1]), 1.0))
            u = noise_np[t, :, 0, :, -1]
            m_prior.append(np.where(rows.numpy(), 1.0, np.abs(u - co["_prior_presence_prob"].numpy()).min(-1)))
            state = SimpleNamespace(z=tuple(_pick(rows, a, b) for a, b in zip(s_obs.z, s_coast.z)),
                                    temporal=_pick(rows, s_obs.temporal, s_coast.temporal), prior=_pick(rows, s_obs.prior, s_coast.prior),
                                    prev_ids=_pick(rows, s_obs.prev_ids, s_coast.prev_ids),
                                    last_id=_pick(rows, s_obs.last_id, s_coast.last_id), t=state.t + 1)
    res = {n: torch.stack(v, 0) for n, v in outs.items()}
    res["presence_margins"] = np.stack(m_post, 0)
    res["prior_margin"] = np.stack(m_prior, 0)
    return res, state
