"""The carried state of a stream, host side, shared by ``SqairStream`` (sqair_amd/stream.py) and ``StreamTrainer`` (sqair_amd/train.py):
a per-row state blob, a source map saying which blob row each particle row of the next step continues (-1: it starts fresh), the
running log-weight sums that follow the rows through that map and, optionally, the buffers of the in-pass SMC resampler that writes
the map (include/sqair_hip.h: sqair_set_state, sqair_set_smc, SqairCarry).  ``SourceMap`` is the host-side policy, NumPy only;
``CarriedState`` adds the device side.  One user registers the state on the handle, the other passes a SqairCarry per call, so
each keeps its own ``step``."""
from __future__ import annotations

import contextlib

import numpy as np


def carried(name):
    """A read-only attribute of a stream class that is its ``carried`` state's attribute ``name``."""
    return property(lambda self: getattr(self.carried, name))


def check_observed(observed, missing, T, B, who, kind):
    """``observed`` of a step of ``who`` (a ``kind``: "stream" / "trainer") as a bool tensor [T', B] (None: every lane has its
    frame); [B] is taken when T' = 1."""
    import torch
    if observed is None:
        return None
    if not missing:
        raise ValueError("{}.step: observed is for a {} with missing=True".format(who, kind))
    m = torch.as_tensor(observed)
    if m.dtype != torch.bool:
        raise ValueError("{}.step: observed must be a bool array, dtype {} given".format(who, m.dtype))
    if T == 1 and tuple(m.shape) == (B,):
        m = m.reshape(1, B)
    if tuple(m.shape) != (T, B):
        raise ValueError("{}.step: observed of shape {} given, [{}, {}] expected{}".format(
            who, tuple(m.shape), T, B, " (or [{}])".format(B) if T == 1 else ""))
    return m


def blank_unobserved(frames, observed):
    """The frames of unobserved lanes as zeros: the pass still computes on them (include/sqair_hip.h: they must be finite)."""
    import torch
    return torch.where(observed.to(frames.device)[:, :, None, None], frames, 0.0)


class SourceMap(object):
    """The pending source map of R = B * K particle rows (K per lane).  ``who``: the class the error texts name."""

    def __init__(self, R, K, who):
        self.R, self.K, self.who = int(R), int(K), who
        self._armed = np.full(self.R, -1, dtype=np.int64)   # the next step's map (None: identity); first: all fresh

    def pending(self):
        return np.arange(self.R, dtype=np.int64) if self._armed is None else self._armed

    def take(self):
        """The armed map, or None for identity; disarms it."""
        m, self._armed = self._armed, None
        return m

    def check_lanes(self, lanes):
        lanes = np.atleast_1d(np.asarray(lanes))
        if lanes.size and (lanes.dtype.kind not in "iu" or lanes.min() < 0 or lanes.max() >= self.R // self.K):
            raise ValueError("{}.reset: lanes must be integers in [0, {})".format(self.who, self.R // self.K))
        return lanes.tolist()

    def check_rows(self, src_rows):
        src = np.asarray(src_rows)
        if src.shape != (self.R,) or src.dtype.kind not in "iu" or (src.size and (src.min() < -1 or src.max() >= self.R)):
            raise ValueError("{}.resample: src_rows must be {} integers in [-1, {})".format(self.who, self.R, self.R))
        return src

    def reset(self, lanes):
        """Lanes (sequences, in [0, B)) whose next step starts a new clip: their K particle rows start fresh, counter 0."""
        m = self.pending().copy()
        for j in self.check_lanes(lanes):
            m[j * self.K:(j + 1) * self.K] = -1
        self._armed = m

    def resample(self, src_rows):
        """Row r of the next step continues row src_rows[r] (-1: starts fresh).  Composes with what was armed before it."""
        src = self.check_rows(src_rows)
        self._armed = np.where(src >= 0, self.pending()[np.maximum(src, 0)], -1)


class CarriedState(SourceMap):
    """The device side: ``state`` (the blob), ``_src`` (the source map the pass reads, frozen into captured graphs),
    ``log_weight_sum`` [R] and, with ``smc``, the resampler's ``log_z``, ``log_evidence``, ``ess``, ``u``, ``resampled`` [B] and its
    ``_uniforms`` input.  With SMC the kernel writes ``_src`` after every pass and nothing is ever armed on the host.  ``ring``: the
    track history's device ring of the last ``history`` steps (``set_history``), or None."""

    def __init__(self, core, B, who, smc):
        import torch
        SourceMap.__init__(self, int(B) * core.K, core.K, who)
        self.core, self.B, self.smc = core, int(B), bool(smc)
        dev = core.device
        z = lambda n, dt=torch.float32: torch.zeros(n, dtype=dt, device=dev)
        with torch.cuda.device(dev):
            self.state = z(core.lib.sqair_state_bytes(core.handle, self.B) // 4)
            self._identity = torch.arange(self.R, dtype=torch.int32, device=dev)
            self._src = self._identity.clone()   # (refreshed before a step that needs another map)
            self.log_weight_sum = z(self.R)
            if self.smc:   # (the first step starts every row fresh)
                self._src.fill_(-1)
                self.log_z, self.log_evidence, self.ess = z(self.B), z(self.B), z(self.B)
                self.u = z(self.B)   # the uniform of each lane's last step
                self.resampled = z(self.B, torch.int32)
                self._uniforms = z(self.B)
                self._armed = None
        self._src_is_identity = True   # (SMC: _src is written on the device only, never refreshed from the host)
        self.ring, self.history, self.history_fields = None, None, ()   # the track history's ring (set_history)

    @staticmethod
    def check_history(L, fields, who):
        """The fields a ring of the last ``L`` steps holds: ``fields`` (of _capi.HISTORY_FIELDS) plus the mandatory three."""
        from . import _capi
        if isinstance(L, bool) or not isinstance(L, (int, np.integer)) or L < 1:
            raise ValueError("{}: history must be an integer >= 1 (the number of steps kept) or None".format(who))
        fields = (fields,) if isinstance(fields, str) else tuple(fields)
        bad = [f for f in fields if f not in _capi.HISTORY_FIELDS]
        if bad:
            raise ValueError("{}: unknown history_fields {} (choose from {})".format(who, bad, tuple(_capi.HISTORY_FIELDS)))
        return tuple(f for f in _capi.HISTORY_FIELDS if f in fields or f in _capi.HISTORY_MANDATORY)

    def set_history(self, L, fields, T):
        """Allocates the zero-filled ring of the last ``L`` steps of ``T`` frames holding ``fields`` (check_history) and returns
        (ring, bytes, field bits) for sqair_set_history."""
        import torch
        from . import _capi
        fields = self.check_history(L, fields, self.who)
        bits = sum(_capi.HISTORY_FIELDS[f] for f in fields)
        core = self.core
        nb = core.lib.sqair_history_bytes(core.handle, int(L), int(T), self.B, bits)
        if nb < 0:
            raise RuntimeError("sqair_history_bytes failed")
        with torch.cuda.device(core.device):
            self.ring = torch.zeros(nb // 4, dtype=torch.int32, device=core.device)
        self.history, self.history_fields = int(L), fields
        return self.ring, nb, bits

    def next_rows(self, src_buf, lw_buf):
        """The rows the next step would start from, on the core's stream: (source map int32 [R], running log weights [R] gathered
        through it).  With SMC these are the resampler's own ``_src`` and ``log_weight_sum`` (already indexed by next-step rows);
        else the pending host-side map is uploaded into ``src_buf`` and the weights that follow it into ``lw_buf``.  What
        ``forecast`` and ``tracks`` start from and weigh by."""
        import torch
        if self.smc:
            return self._src, self.log_weight_sum
        src_buf.copy_(torch.as_tensor(self.pending().astype(np.int32)), non_blocking=True)
        keep = src_buf >= 0
        lw_buf.copy_(torch.where(keep, self.log_weight_sum[src_buf.long().clamp_min(0)], torch.zeros_like(lw_buf)))
        return src_buf, lw_buf

    def adopt(self, state):
        """Hand-over: the first step continues every row of the given blob (copied)."""
        import torch
        state = torch.as_tensor(state)
        if state.dtype != torch.float32 or state.numel() != self.state.numel():
            raise ValueError("{}: state must be a float32 blob of sqair_state_bytes(core, B) = {} bytes".format(
                self.who, self.state.numel() * 4))
        with torch.cuda.device(self.core.device):
            self.state.copy_(state.reshape(-1))
            self._src.copy_(self._identity)
        self._armed = None

    @contextlib.contextmanager
    def _on_core_stream(self):
        """Device selected, the core's stream current and joined with the caller's on the way in and out."""
        import torch
        core = self.core
        with torch.cuda.device(core.device):
            core._join_in()
            with core.on_stream():
                yield
            core._join_out()

    def reset(self, lanes):
        if not self.smc:
            return SourceMap.reset(self, lanes)
        lanes, K = self.check_lanes(lanes), self.K
        with self._on_core_stream():   # after the map the last step's resampler wrote: the lane's rows fresh, its weights zero
            for j in sorted(set(lanes)):
                self._src[j * K:(j + 1) * K].fill_(-1)
                self.log_weight_sum[j * K:(j + 1) * K].zero_()
                self.log_z[j:j + 1].zero_()

    def resample(self, src_rows):
        """With SMC on it composes on the device with the map the last step's resampler wrote: src_new[r] = src[src_rows[r]].  The
        running log-weight sums follow the rows."""
        if not self.smc:
            return SourceMap.resample(self, src_rows)
        import torch
        src = self.check_rows(src_rows)
        with self._on_core_stream():
            s = torch.as_tensor(src.astype(np.int64)).pin_memory().to(self.core.device, non_blocking=True)
            keep = s >= 0
            s = s.clamp_min(0)
            self._src.copy_(torch.where(keep, self._src[s], torch.full_like(self._src, -1)))
            self.log_weight_sum.copy_(torch.where(keep, self.log_weight_sum[s], torch.zeros_like(self.log_weight_sum)))

    def feed(self, frames, noise, uniforms, seed, frame, **shard):
        """A step's inputs, on the core's stream: the frames, the noise (given, or Philox keyed by (seed, frame, **shard: the
        position in the global batch)), the resampler's uniforms, the source map (``upload``)."""
        core = self.core
        core.obs.copy_(frames, non_blocking=True)
        if noise is not None:
            core.noise.copy_(noise.reshape(core.noise.shape), non_blocking=True)
        else:
            core.draw_noise(seed=seed, step=frame, **shard)
        if uniforms is not None:
            self._uniforms.copy_(uniforms, non_blocking=True)
        self.upload()

    def upload(self):
        """The armed map into ``_src`` and ``log_weight_sum`` gathered through it, else the identity map restored once.  (SMC:
        nothing is armed; the map is the one the last step's resampler wrote.)"""
        import torch
        armed = self.take()
        if armed is not None:
            dev = self.core.device
            m = torch.as_tensor(armed.astype(np.int32))
            self._src.copy_(m, non_blocking=True)
            lw = self.log_weight_sum[torch.as_tensor(np.maximum(armed, 0), device=dev)]
            self.log_weight_sum.copy_(torch.where(m.to(dev) >= 0, lw, torch.zeros_like(lw)))
            self._src_is_identity = False
        elif not self._src_is_identity:
            self._src.copy_(self._identity)
            self._src_is_identity = True

    def smc_struct(self, ess_frac, seed, with_uniforms):
        """The ``_capi.SqairSmc`` naming these buffers; the lane uniforms read from ``_uniforms`` or drawn by Philox."""
        from . import _capi
        return _capi.SqairSmc(ess_frac=ess_frac, seed=seed & 0xFFFFFFFFFFFFFFFF,
                              uniforms=self._uniforms.data_ptr() if with_uniforms else None, log_w=self.log_weight_sum.data_ptr(),
                              log_z=self.log_z.data_ptr(), log_evidence=self.log_evidence.data_ptr(), ess=self.ess.data_ptr(),
                              u_out=self.u.data_ptr(), resampled=self.resampled.data_ptr(), src_rows=self._src.data_ptr())

    def check_inputs(self, T, frames, noise, uniforms, kind):
        """A step's ``frames`` [T, B, H, W], ``noise`` (core.noise's size) and ``uniforms`` [B] (SMC only) as float32 tensors."""
        import torch
        core, fn = self.core, self.who + ".step"
        frames = torch.as_tensor(frames, dtype=torch.float32)
        if frames.dim() == 5:
            frames = frames[..., 0]
        if tuple(frames.shape) != (T, self.B, core.H, core.W):
            raise ValueError("{}: frames of shape {} given, [{}, {}, {}, {}] expected".format(
                fn, tuple(frames.shape), T, self.B, core.H, core.W))
        if noise is not None:
            noise = torch.as_tensor(noise, dtype=torch.float32)
            if noise.numel() != core.noise.numel():
                raise ValueError("{}: noise of shape {} given, {} expected".format(fn, tuple(noise.shape), tuple(core.noise.shape)))
        if uniforms is not None:
            if not self.smc:
                raise ValueError("{}: uniforms are for a {} with resample='systematic'".format(fn, kind))
            uniforms = torch.as_tensor(uniforms, dtype=torch.float32)
            if tuple(uniforms.shape) != (self.B,):
                raise ValueError("{}: uniforms of shape {} given, [{}] expected".format(fn, tuple(uniforms.shape), self.B))
        return frames, noise, uniforms
