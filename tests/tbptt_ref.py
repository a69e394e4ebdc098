"""fp64 reference of a carried training chunk (include/sqair_hip.h: SqairCarry): the oracle's ``sequence`` from a carried state,
and the target of the reference's make_target on the chunk alone -- VIMCO over the chunk's log weights and discrete log-probs, / T'.
The state a chunk starts from is detached: no gradient flows into it, as on the device."""
from types import SimpleNamespace

import numpy as np
import torch

from oracle import sqair_oracle as O


def detach_state(state):
    return SimpleNamespace(**{k: tuple(x.detach() for x in v) if isinstance(v, tuple) else v.detach() for k, v in vars(state).items()})


def chunk_target(orc, frames, noise, K, state=None):
    """frames [T', B, H, W]; noise [T', B*K, 2, N, nzw]; state: the rows' start (None: fresh).  Returns (target, outputs, state
    after the chunk)."""
    frames = torch.as_tensor(np.asarray(frames), dtype=orc.dtype)
    T, B = int(frames.shape[0]), int(frames.shape[1])
    tiled = O.tile_input_for_iwae(frames, K)
    out, st = orc.sequence(tiled, torch.as_tensor(np.asarray(noise), dtype=orc.dtype),
                           state=None if state is None else detach_state(state), return_state=True)
    log_w = out["log_weights_per_timestep"].sum(0).reshape(B, K)
    target = O.vimco(log_w, out["discrete_log_prob"].sum(0)) / float(T)
    return target, out, st
