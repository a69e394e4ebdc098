"""Train-step semantics of the reference driver, host side.

reference: sqair/scripts/experiment.py:126-155 — global step, piecewise-constant learning rate
(``schedule`` = comma-separated relative segment lengths; the rate is divided by 3 at every boundary),
``tf.train.RMSPropOptimizer(lr, momentum=.9)``; sqair/data/mnist_tools.py:84-92 — sequence-length
curriculum (``seq_len`` grows by one every ``stage_itr`` iterations).  The parameter update itself is the
fused HIP kernel ``sqair_rmsprop_step``; the gradients come from ``sqair_backward`` (csrc/sqair_train.hip).
``Optimizer`` mirrors the ``opt.compute_gradients`` / ``opt.apply_gradients`` pair the reference's ``make_target``
and driver use; ``Trainer`` is the driver's inner loop (experiment.py:150-185) for one rank."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .carried import CarriedState, blank_unobserved, carried, check_observed


def lr_schedule(F):
    """Returns (boundaries, values) of the piecewise-constant learning rate (experiment.py:127-138):
    schedule '4,6,10' over train_itr iterations -> boundaries at cumulative 4/20 and 10/20 of train_itr,
    values lr, lr/3, lr/9."""
    sched = [float(s) for s in str(F.schedule).split(",")]
    total = sum(sched)
    bounds = [int(round(v)) for v in (np.cumsum(sched)[:-1] / total * int(F.train_itr))]
    values = [float(F.learning_rate) * (1.0 / 3.0) ** i for i in range(len(sched))]
    return bounds, values


def learning_rate(F, step):
    bounds, values = lr_schedule(F)
    # tf.train.piecewise_constant: values[0] for x <= boundaries[0], values[i] for boundaries[i-1] < x <= boundaries[i]
    i = int(np.searchsorted(np.asarray(bounds), step, side="left"))
    return values[i]


def curriculum_seq_len(F, step, max_len):
    """Sequence-length curriculum (mnist_tools.py:84-92): seq_len + step // stage_itr, capped at the data length;
    seq_len = 0 or stage_itr = 0 disables it."""
    if int(F.seq_len) <= 0 or int(F.stage_itr) <= 0:
        return int(max_len)
    return int(min(max_len, int(F.seq_len) + step // int(F.stage_itr)))


def rmsprop_reference(theta, grad, ms, mom, lr, decay=0.9, momentum=0.9, eps=1e-10):
    """NumPy restatement of the TF update used by the tests."""
    ms = decay * ms + (1.0 - decay) * grad * grad
    mom = momentum * mom + lr * grad / np.sqrt(ms + eps)
    return theta - mom, ms, mom


class Optimizer(object):
    """The optimisers the reference driver offers (experiment.py:139-147) on the flat fp32 buffers of a ``SqairCore``.
    ``rmsprop`` (the default and the only one the shipped configs use) is the fused HIP kernel; ``adam`` / ``sgd`` /
    ``momentum`` are a handful of elementwise torch ops on the same device buffers (TF1 defaults)."""

    def __init__(self, core, kind="rmsprop", momentum=0.9, decay=0.9, epsilon=1e-10):
        import torch
        self.core, self.kind = core, str(kind).lower()
        if self.kind not in ("rmsprop", "adam", "sgd", "momentum"):
            raise ValueError("unknown optimiser {!r}".format(kind))
        self.momentum, self.decay, self.epsilon = float(momentum), float(decay), float(epsilon)
        # TF initialises the RMSProp mean-square slot with ones, Adam's second moment with zeros
        self.ms = torch.ones_like(core.flat) if self.kind == "rmsprop" else torch.zeros_like(core.flat)
        self.mom = torch.zeros_like(core.flat)
        self.t = 0

    def compute_gradients(self, model, l2_reg=0.0):
        """``opt.compute_gradients(target)`` of the reference (model.py:159-161): evaluates the VIMCO target and the gradient
        of every trainable variable for the model's current batch; returns the (gradient, variable name) list."""
        return model.make_target(self, l2_reg=l2_reg)[1]

    def apply_gradients(self, grads, lr=None, grad_scale=1.0, global_step=None):
        """theta <- theta - update(grad_scale * grad); re-packs the weights for the next forward pass.  ``grads`` is the
        core's flat gradient tensor or the (gradient, name) list ``Model.make_target`` / ``compute_gradients`` return (its
        entries are views of that flat tensor).  ``lr`` defaults to the piecewise schedule of the core's flags at
        ``global_step`` (experiment.py:127-138; default: the number of updates applied so far)."""
        import torch
        from . import _capi
        core = self.core
        if isinstance(grads, (list, tuple)):
            if len(grads) != len(core.spec):
                raise ValueError("expected one (gradient, name) pair per variable ({}), got {}".format(len(core.spec), len(grads)))
            flat_grad = core.flat_grad
        else:
            flat_grad = grads
        if lr is None:
            lr = learning_rate(core.F, self.t if global_step is None else int(global_step))
        self.t += 1
        if self.kind == "rmsprop":
            with torch.cuda.device(core.device):
                core.check(core.lib.sqair_rmsprop_step(
                    core.handle, core.flat.data_ptr(), flat_grad.data_ptr(), self.ms.data_ptr(), self.mom.data_ptr(),
                    core.n_params, float(lr), self.decay, self.momentum, self.epsilon, float(grad_scale),
                    C.c_void_p(torch.cuda.current_stream(core.device).cuda_stream)), "sqair_rmsprop_step")
        else:
            g = flat_grad * float(grad_scale) if grad_scale != 1.0 else flat_grad
            if self.kind == "sgd":
                core.flat.add_(g, alpha=-float(lr))
            elif self.kind == "momentum":      # tf.train.MomentumOptimizer: accum = m accum + g; theta -= lr accum
                self.mom.mul_(self.momentum).add_(g)
                core.flat.add_(self.mom, alpha=-float(lr))
            else:                              # tf.train.AdamOptimizer defaults beta1 .9, beta2 .999, eps 1e-8
                b1, b2, eps = 0.9, 0.999, 1e-8
                self.mom.mul_(b1).add_(g, alpha=1.0 - b1)
                self.ms.mul_(b2).addcmul_(g, g, value=1.0 - b2)
                lr_t = float(lr) * np.sqrt(1.0 - b2 ** self.t) / (1.0 - b1 ** self.t)
                core.flat.addcdiv_(self.mom, self.ms.sqrt().add_(eps), value=-lr_t)
        core.pack()


def _finish_step(tr, g):
    """The tail of a training step of ``tr`` (a ``Trainer`` or a ``StreamTrainer``), on the core's stream: the l2 term, the all-reduce
    of the flat gradient ``g`` over the ranks (the single collective of the step), the optimiser, the step count."""
    from .dist import allreduce_flat_grads
    core, F = tr.core, tr.F
    l2 = float(getattr(F, "l2", 0.0))
    if l2 != 0.0:
        core.check(core.lib.sqair_add_l2_grad(
            core.handle, core.flat.data_ptr(), g.data_ptr(), core.n_params, l2, core._stream()), "sqair_add_l2_grad")
    scale = allreduce_flat_grads(g, comm=tr.comm, stream=core.stream) if tr.collective else 1.0
    tr.opt.apply_gradients(g, learning_rate(F, tr.step_no), grad_scale=scale)
    tr.step_no += 1


class Trainer(object):
    """One rank of the reference's training loop (experiment.py:150-185): per step draw noise, evaluate the VIMCO
    target and its gradients on this rank's shard of sequences (ONE HIP graph replay), all-reduce the flat gradient
    buffer over the ranks (the single collective of the step, RCCL over xGMI), apply the optimiser.
    ``model`` is a ``sqair_amd.model.Model`` bound to this rank's shard."""

    def __init__(self, model, F, use_graph=True, comm=None, collective=True):
        """comm: a ``sqair_amd.rccl.RcclComm`` — the gradient all-reduce is then enqueued on the core's own stream
        (``ncclAllReduce``); None = the default ``torch.distributed`` group, if one is initialised.  ``collective=False``: a
        trainer that belongs to ONE rank of a running job (bench.py's single-GPU reference and timeline legs) and must not
        enter the job's collective."""
        self.model, self.core, self.F = model, model.core, F
        self.comm = comm
        self.collective = bool(collective)
        self.opt = Optimizer(self.core, getattr(F, "opt", "rmsprop"))
        self.step_no = 0
        self.use_graph = bool(use_graph)

    def step(self, obs=None, noise=None, generator=None, seed=None, global_batch=None, b0=0, presence=None):
        """One training step, asynchronous on the core's stream (``core.stream.synchronize()`` or read metrics inside
        ``core.on_stream()`` to observe results).  Returns the flat gradient buffer: on a multi-rank job it holds the SUM over
        the ranks of the shard gradients (the all-reduce's result); the 1 / world that makes it the reference's ``reduce_mean``
        over the global batch is applied inside the optimiser kernel (``grad_scale``), so a caller that logs or clips these
        values must scale them by ``1 / world`` itself."""
        import torch
        core = self.core
        if obs is not None:
            obs = torch.as_tensor(obs, dtype=torch.float32)
            if obs.dim() == 5:
                obs = obs[..., 0]
            if int(obs.shape[0]) != core.T or int(obs.shape[1]) != core.B:
                # sequence-length curriculum (mnist_tools.py:80-92) or a new batch size: re-bind through the Model so that
                # its n_timesteps / batch_size / obs / ground truth follow (the gradient graph is re-captured on the next
                # evaluation)
                self.model.rebind(obs, presence=presence)
                obs = None
            else:
                self.model.obs = obs.to(core.device)
                if presence is not None:
                    self.model.gt_presence = torch.as_tensor(presence, dtype=torch.float32).to(core.device)
        with core.on_stream():
            if obs is not None:
                core.obs.copy_(self.model.obs.reshape(core.obs.shape))
            if noise is not None:
                core.noise.copy_(torch.as_tensor(noise, dtype=torch.float32).reshape(core.noise.shape))
            elif seed is not None:  # library Philox keyed by (seed, step, position in the global batch)
                core.draw_noise(seed=seed, step=self.step_no, global_batch=global_batch, b0=b0)
            else:
                core.draw_noise(generator)
            g = core.grad_step(use_graph=self.use_graph)
            _finish_step(self, g)
        return g


class StreamTrainer(object):
    """Training on a stream, chunk by chunk: truncated BPTT with a carried state (include/sqair_hip.h: SqairCarry), the
    ``SqairStream`` idiom for training.  Every ``step(frames)`` takes the next T' = frames_per_step frames of B lanes, starts each
    particle row from the state the previous step left (the first step starts every row fresh), evaluates the chunk's VIMCO
    target / T' and its gradient with the imported state held constant, applies l2, the all-reduce and the optimiser exactly as
    ``Trainer.step`` does, and keeps frame T''s state (records, cell states, ids, counters) in ``state`` for the next step.

    ``resample="systematic"``: the forward ends with the SMC resampler at ess_frac = 1 (every lane, every chunk boundary), so the
    sum of a lane's chunk elbo_iwae is its SMC log evidence (``log_evidence``), the FIVO bound; ``ess`` and ``ancestors`` (the next
    step's source map) as in ``SqairStream``.  Default noise: the library's Philox keyed by (seed, index of the chunk's first frame,
    position in the global batch), so that data-parallel ranks draw what one GPU would.  ``state`` can be handed to
    ``SqairStream(core, B, state=...)`` of the same core and B.  The trainer takes no registration on the handle: close a
    ``SqairStream`` of the same core before stepping.

    ``missing=True``: a step takes ``observed`` [T', B] (include/sqair_hip.h: "training on gappy and ragged streams").  A lane
    without a frame -- a dropped frame, a slower camera, or, as a trailing run, a clip that ends inside the chunk -- coasts on the
    prior: its log weight is 0, its posterior gets no gradient, the prior is trained through the coasted draws and their score term.
    The step then runs the masked pair of calls (T' + 1 launches more each way); the mask lives in one device buffer that the
    captured graph reads, so every pattern replays the same graph.  On a data-parallel job the mask covers this rank's lanes."""

    def __init__(self, core_or_model, F, B, frames_per_step=1, seed=0, resample=None, use_graph=True, comm=None, collective=True,
                 outputs=("what", "where", "presence", "obj_id"), missing=False):
        core = getattr(core_or_model, "core", core_or_model)
        if core.cfg.sample_from_prior:
            raise ValueError("StreamTrainer: generation modes (sample_from_prior) do not carry a state")
        if resample not in (None, "systematic"):
            raise ValueError("StreamTrainer: resample must be None or 'systematic'")
        self.core, self.F = core, F
        self.B, self.K, self.T = int(B), core.K, int(frames_per_step)
        if self.B < 1 or self.T < 1:
            raise ValueError("StreamTrainer: B and frames_per_step must be >= 1")
        self.R = self.B * self.K
        self.smc = resample is not None
        self.seed = int(seed)
        self.comm, self.collective, self.use_graph = comm, bool(collective), bool(use_graph)
        self.opt = Optimizer(core, getattr(F, "opt", "rmsprop"))
        self.step_no = 0
        self.frame = 0          # frames consumed so far
        names = ["log_weights_per_timestep", "discrete_log_prob", "data_ll_per_sample", "kl_per_sample",
                 "log_q_z_given_x_per_sample", "log_p_z_per_sample", "num_steps_per_sample", "num_disc_steps_per_sample",
                 "num_prop_steps_per_sample"]
        core.bind(self.T, self.B, names + [n for n in outputs if n not in names])
        # the blob, the source map (host-side until a step uploads it; SMC: the resampler's) and the weights (sqair_amd/carried.py)
        self.carried = CarriedState(core, self.B, "StreamTrainer", self.smc)
        self._carries = {}      # SqairCarry (and its SqairSmc) per uniforms mode, kept alive while the trainer lives
        self.missing = bool(missing)
        if self.missing:   # the device mask [T', B] both masked calls read: all observed until a step says otherwise
            import torch
            self._observed = torch.ones((self.T, self.B), dtype=torch.int32, device=core.device)
            self._observed_is_ones = True
        core.stream.synchronize()

    # the carried state's, read-only; ``ancestors`` (SMC): the source map of the next step, written by the resampler
    state, log_weight_sum, log_z, log_evidence, ess, u, resampled, ancestors = (
        carried(n) for n in ("state", "log_weight_sum", "log_z", "log_evidence", "ess", "u", "resampled", "_src"))

    def _carry(self, uniforms):
        from . import _capi
        c = self._carries.get(uniforms)
        if c is None:
            cs = self.carried
            smc = cs.smc_struct(1.0, self.seed, uniforms) if self.smc else None
            c = _capi.SqairCarry(state_in=cs.state.data_ptr(), state_out=cs.state.data_ptr(), src_rows=cs._src.data_ptr(),
                                 state_bytes=cs.state.numel() * 4, B=self.B, smc=C.pointer(smc) if smc is not None else None)
            self._carries[uniforms] = c
            c._smc = smc   # (the SqairSmc the pointer names lives as long as the carry)
        return c

    # ---- source map (SqairStream's semantics) ------------------------------------------------------------------------------
    def reset(self, lanes):
        """Lanes (in [0, B)) whose next step starts a new clip: their K particle rows start fresh, counter 0."""
        self.carried.reset(lanes)

    def resample(self, src_rows):
        """Row r of the next step continues row src_rows[r] (-1: fresh); composes with a reset armed before it.  Not with SMC (the
        resampler writes the map)."""
        if self.smc:
            raise ValueError("StreamTrainer.resample: the SMC resampler writes the source map (resample='systematic')")
        self.carried.resample(src_rows)

    # ---- stepping ------------------------------------------------------------------------------------------------------------
    def _check_observed(self, observed):
        return check_observed(observed, self.missing, self.T, self.B, "StreamTrainer", "trainer")

    def step(self, frames, noise=None, seed=None, uniforms=None, global_batch=None, b0=0, observed=None):
        """One training step on the next chunk: frames [T', B, H, W]; ``noise`` [T', B*K, 2, N, 4 + n_what + 1] (default: Philox
        keyed by (``seed`` or the trainer's seed, the chunk's first frame, position in the global batch ``global_batch`` / ``b0``));
        ``uniforms`` [B] (SMC only: the resampler's uniforms; default Philox).  Asynchronous on the core's stream.  Returns the
        flat gradient buffer after the optimiser step (on a multi-rank job the SUM over the ranks, as ``Trainer.step``).
        ``observed`` (trainers with ``missing=True``): bool [T', B] of this rank's lanes, or [B] when T' = 1; False = the lane has no
        frame there and coasts on the prior.  Its frame is replaced by zeros, so it may hold anything, NaN included.  Default:
        every lane observed."""
        observed = self._check_observed(observed)   # (before the core is touched)
        core, cs = self.core, self.carried
        frames, noise, uniforms = cs.check_inputs(self.T, frames, noise, uniforms, "trainer")
        if observed is not None:
            if frames.is_cuda:
                observed = observed.to(frames.device)
            frames = blank_unobserved(frames, observed)
        with core.on_stream():
            cs.feed(frames, noise, uniforms, self.seed if seed is None else int(seed), self.frame, global_batch=global_batch, b0=b0)
            if self.missing:
                if observed is not None:
                    self._observed.copy_(observed.to(core.device, non_blocking=True))
                elif not self._observed_is_ones:
                    self._observed.fill_(1)
                self._observed_is_ones = observed is None
            g = core.grad_step_carry(self._carry(uniforms is not None), use_graph=self.use_graph,
                                     observed=self._observed if self.missing else None)
            if not self.smc:
                cs.log_weight_sum += core.out["log_weights_per_timestep"].sum(0)
            _finish_step(self, g)
        self.frame += self.T
        return g
