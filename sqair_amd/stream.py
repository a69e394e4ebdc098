"""Stateful streaming inference: a video fed as its frames arrive, object identities and latent states carried from call to call.

``SqairStream(core, B)`` owns a state blob on the device (include/sqair_hip.h: sqair_state_bytes / sqair_set_state) and runs the
T'-frame inference pass of ``core`` (frames_per_step = T') once per ``step()``: each particle row starts from the state the
previous step left and the pass writes its new state back into the same blob.  With ``use_graph`` ONE HIP graph of that pass is
captured on the first step and replayed on every later one -- the rows' frame counters live on the device, so the same graph
serves frame 0, frame 1000 and a batch in which some lanes were just reset.

Stepping a sequence in chunks gives the results of one pass over the whole sequence, bit for bit, when the chunks see the same
noise (tests/test_stream_state.py).  Without explicit ``noise`` a step draws its own from the library's Philox generator keyed by
(seed, frame index of the step's first frame, row): NOT the draws a whole-sequence pass with the same seed makes (that one keys
every frame of the pass by one step index), so results agree with such a pass only in distribution.

The stream takes over its core's handle: while it is open, every inference pass of that handle carries the state.  ``close()``
hands the handle back.
"""
from __future__ import annotations

import numpy as np
import torch

DEFAULT_OUTPUTS = ("what", "where", "presence", "obj_id", "log_weights_per_timestep")


class SqairStream(object):
    def __init__(self, core, B, frames_per_step=1, outputs=DEFAULT_OUTPUTS, use_graph=True, seed=0):
        if core.cfg.sample_from_prior:
            raise ValueError("SqairStream: generation modes (sample_from_prior) do not carry a state across calls")
        self.core = core
        self.B, self.K = int(B), core.K
        self.R = self.B * self.K
        self.T = int(frames_per_step)
        if self.B < 1 or self.T < 1:
            raise ValueError("SqairStream: B and frames_per_step must be >= 1")
        outputs = tuple(outputs)
        if "log_weights_per_timestep" not in outputs:   # (the running log-weight sums)
            outputs = outputs + ("log_weights_per_timestep",)
        self.outputs = outputs
        self.use_graph = bool(use_graph)
        self.seed = int(seed)
        self.frame = 0          # frames consumed so far (host side; the rows' own counters are in the blob)
        lib, dev = core.lib, core.device
        core.bind(self.T, self.B, list(outputs))
        with torch.cuda.device(dev):
            self.state = torch.zeros(lib.sqair_state_bytes(core.handle, self.B) // 4, dtype=torch.float32, device=dev)
            self._identity = torch.arange(self.R, dtype=torch.int32, device=dev)
            self._src = self._identity.clone()   # (frozen into the captured graph; refreshed before a step that needs another map)
            self.log_weight_sum = torch.zeros(self.R, dtype=torch.float32, device=dev)
        self._src_is_identity = True
        self._armed = np.full(self.R, -1, dtype=np.int64)   # host-side source map of the next step (None: identity); first: all fresh
        self._graph = False
        core.stream.synchronize()
        core.check(lib.sqair_set_state(core.handle, self.state.data_ptr(), self.state.data_ptr(), self._src.data_ptr(),
                                       self.state.numel() * 4, self.B), "sqair_set_state")
        core._graph_ready = False   # (the handle's graph is now this stream's)

    # ---- source map -------------------------------------------------------------------------------------------------------
    def _pending(self):
        return np.arange(self.R, dtype=np.int64) if self._armed is None else self._armed

    def reset(self, lanes):
        """Lanes (sequences, in [0, B)) whose next step starts a new clip: their K particle rows start fresh, counter 0."""
        lanes = np.atleast_1d(np.asarray(lanes))
        if lanes.size and (lanes.dtype.kind not in "iu" or lanes.min() < 0 or lanes.max() >= self.B):
            raise ValueError("SqairStream.reset: lanes must be integers in [0, {})".format(self.B))
        m = self._pending().copy()
        for j in lanes.tolist():
            m[j * self.K:(j + 1) * self.K] = -1
        self._armed = m

    def resample(self, src_rows):
        """Row r of the next step continues row src_rows[r] (-1: starts fresh); e.g. SMC resampling of the particles of each
        sequence, src[b*K + k] = b*K + k'.  Composes with a reset armed before it.  The running log-weight sums follow the rows."""
        src = np.asarray(src_rows)
        if src.shape != (self.R,) or src.dtype.kind not in "iu" or (src.size and (src.min() < -1 or src.max() >= self.R)):
            raise ValueError("SqairStream.resample: src_rows must be {} integers in [-1, {})".format(self.R, self.R))
        m = self._pending()
        self._armed = np.where(src >= 0, m[np.maximum(src, 0)], -1)

    # ---- stepping ---------------------------------------------------------------------------------------------------------
    def step(self, frames, noise=None, seed=None):
        """Consumes frames [T', B, H, W] (T' = frames_per_step); returns this step's per-frame outputs {name: [T', B*K, ...]}
        (copies, valid on the current stream).  ``noise`` [T', B*K, 2, N, 4 + n_what + 1]; default: the library's generator
        keyed by (``seed`` or the stream's seed, frame index)."""
        core = self.core
        frames = torch.as_tensor(frames, dtype=torch.float32)
        if frames.dim() == 5:
            frames = frames[..., 0]
        if tuple(frames.shape) != (self.T, self.B, core.H, core.W):
            raise ValueError("SqairStream.step: frames of shape {} given, [{}, {}, {}, {}] expected".format(
                tuple(frames.shape), self.T, self.B, core.H, core.W))
        if noise is not None:
            noise = torch.as_tensor(noise, dtype=torch.float32)
            if noise.numel() != core.noise.numel():
                raise ValueError("SqairStream.step: noise of shape {} given, {} expected".format(tuple(noise.shape),
                                                                                               tuple(core.noise.shape)))
        lib = core.lib
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                core.obs.copy_(frames, non_blocking=True)
                if noise is not None:
                    core.noise.copy_(noise.reshape(core.noise.shape), non_blocking=True)
                else:
                    core.draw_noise(seed=self.seed if seed is None else int(seed), step=self.frame)
                if self._armed is not None:
                    m = torch.as_tensor(self._armed.astype(np.int32))
                    self._src.copy_(m, non_blocking=True)
                    lw = self.log_weight_sum[torch.as_tensor(np.maximum(self._armed, 0), device=core.device)]
                    self.log_weight_sum.copy_(torch.where(m.to(core.device) >= 0, lw, torch.zeros_like(lw)))
                    self._src_is_identity = False
                    self._armed = None
                elif not self._src_is_identity:
                    self._src.copy_(self._identity)
                    self._src_is_identity = True
                if self.use_graph:
                    if not self._graph:
                        core.stream.synchronize()
                        core.check(lib.sqair_graph_capture(*core._args(0)), "sqair_graph_capture")
                        self._graph = True
                    core.check(lib.sqair_graph_launch(core.handle, core._stream()), "sqair_graph_launch")
                else:
                    core.check(lib.sqair_forward(*core._args(0)), "sqair_forward")
                out = {k: core.out[k].clone() for k in self.outputs}
                self.log_weight_sum += out["log_weights_per_timestep"].sum(0)
            core._join_out()
        self.frame += self.T
        return out

    def close(self):
        """Switches the carried state off on the core's handle (its passes start from the initial state again)."""
        core = self.core
        if core.handle:
            core.stream.synchronize()
            core.check(core.lib.sqair_set_state(core.handle, None, None, None, 0, 0), "sqair_set_state")
            core._graph_ready = False
