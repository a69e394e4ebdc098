"""fp64 reference of a masked carried training chunk (include/sqair_hip.h: "training on gappy and ragged streams"): a
differentiable chunk target, composed of the pieces tests/coast_ref.py uses -- ``orc.sequence`` one frame at a time for observed
rows, ``coast_ref.prior_frame`` (propagate_prior, compute_object_ids, select_present) for unobserved ones, ``torch.where`` on the
mask -- and of tests/tbptt_ref.py: the start state detached, ``O.vimco(log_w, disc_lp) / T'``.  Nothing runs under no_grad.

A coasted (frame, row) has log weight 0.  Its discrete log-prob is the score term of the presences the prior drew,
sum_slots pres log sigmoid(l) + (1 - pres) log sigmoid(-l), when the lane has an observed frame later in the chunk, else 0.

    target, out, state = chunk_target(orc, frames, noise, K, observed, state=None)
"""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import sqair_oracle as O
from tests import coast_ref as CR
from tests.hip_util import presence_margins
from tests.tbptt_ref import detach_state


def later_observed(observed):
    """[T, B] bool: the lane has an observed frame after frame t of the chunk."""
    observed = np.asarray(observed, dtype=bool)
    later = np.zeros_like(observed)
    for t in range(observed.shape[0] - 1):
        later[t] = observed[t + 1:].any(0)
    return later


def score_term(pres, logit):
    """Bernoulli log-probability of the drawn presences under the coasted logits, summed over the slots.  [B', N] -> [B']."""
    ls = torch.nn.functional.logsigmoid
    return (pres * ls(logit) + (1.0 - pres) * ls(-logit)).sum(-1)


def chunk_target(orc, frames, noise, K, observed, state=None, score=True, detach_draws=False):
    """frames [T', B, H, W]; noise [T', B*K, 2, N, nzw]; observed [T', B] bool; state: the rows' start (None: fresh).
    ``score=False`` leaves the score term out, ``detach_draws=True`` cuts the gradient through the coasted what / where draws: the
    two variants a test uses to show that it can see each of the two paths.  Returns (target, {name: [T', B', ...]} as
    coast_ref's plus ``presence_margins`` / ``prior_margin`` [T', B'], the state after the chunk)."""
    dt = orc.dtype
    frames = torch.as_tensor(np.asarray(frames), dtype=dt)
    T, B = int(frames.shape[0]), int(frames.shape[1])
    observed = np.asarray(observed, dtype=bool)
    assert observed.shape == (T, B), observed.shape
    later = later_observed(observed)
    tiled = O.tile_input_for_iwae(frames, K)
    noise_np = np.asarray(noise)
    noise = torch.as_tensor(noise_np, dtype=dt)
    state = orc.initial_state(B * K) if state is None else detach_state(state)
    outs, m_post, m_prior = {}, [], []
    zero = torch.zeros((), dtype=dt)
    for t in range(T):
        rows = torch.as_tensor(np.repeat(observed[t], K))
        rows_later = torch.as_tensor(np.repeat(later[t], K))
        img = torch.where(rows[:, None, None], tiled[t], zero)     # (what the trainer feeds; never matters)
        so, s_obs = orc.sequence(img[None], noise[t:t + 1], state=state, return_state=True)
        co, s_coast = CR.prior_frame(orc, state, noise[t, :, 0])
        if detach_draws:
            what, where, pres, logit = s_coast.z
            s_coast.z = (what.detach(), where.detach(), pres, logit)
        co["discrete_log_prob"] = torch.where(rows_later, score_term(co["presence"], co["presence_logit"]), zero) if score else None
        for n, v in so.items():
            if n.startswith("_"):
                continue
            v = v[0]
            alt = co.get(n) if n in CR.COASTED + CR.COUNTS + ("discrete_log_prob",) else None
            outs.setdefault(n, []).append(CR._pick(rows, v, torch.zeros_like(v) if alt is None else alt))
        m_post.append(np.where(rows.numpy(), presence_margins(so, noise_np[t:t + 1]), 1.0))
        u = noise_np[t, :, 0, :, -1]
        m_prior.append(np.where(rows.numpy(), 1.0, np.abs(u - co["_prior_presence_prob"].detach().numpy()).min(-1)))
        state = SimpleNamespace(z=tuple(CR._pick(rows, a, b) for a, b in zip(s_obs.z, s_coast.z)),
                                temporal=CR._pick(rows, s_obs.temporal, s_coast.temporal), prior=CR._pick(rows, s_obs.prior, s_coast.prior),
                                prev_ids=CR._pick(rows, s_obs.prev_ids, s_coast.prev_ids),
                                last_id=CR._pick(rows, s_obs.last_id, s_coast.last_id), t=state.t + 1)
    res = {n: torch.stack(v, 0) for n, v in outs.items()}
    log_w = res["log_weights_per_timestep"].sum(0).reshape(B, K)
    target = O.vimco(log_w, res["discrete_log_prob"].sum(0)) / float(T)
    res["presence_margins"] = np.stack(m_post, 0)
    res["prior_margin"] = np.stack(m_prior, 0)
    return target, res, state
