"""Optimisers, learning-rate schedules and the gradient all-reduce of the LiDOG step on flat HBM buffers.

Restates what the reference configures through pytorch-lightning (python the GPU box never receives):
  configure_optimizers  utils/pipelines/trainer_lighting_2d.py:349-394, utils/pipelines/trainer_lighting.py:335-380
      Adam(lr, weight_decay=1e-4)  |  SGD(lr, momentum=0.98, weight_decay=1e-4, nesterov=True)      (:26-27,351-360)
      CosineAnnealingLR(T_max=10) | ExponentialLR(gamma=0.99) | CyclicLR(lr/1e4 .. lr, step_size_up=5,
      mode="triangular2", cycle_momentum=False)                                                        (:379-389)
      returned as ([optimizer], [scheduler]) => Lightning steps the scheduler once per training EPOCH
  DDP gradient averaging  train_lidog.py:227-231 (strategy='ddp')

Parameters, gradients and optimiser state live in contiguous fp32 buffers: one fused HIP kernel per step
(csrc/optim.hip:k_adam, csrc/optim.hip:k_sgd), one RCCL all-reduce per 32 MiB bucket.

Beyond the reference, on the same flat buffers: WeightAverage (EMA / SWA, csrc/wavg.hip), and the global gradient norm
with its two users, clip_grad_norm (Lightning's gradient_clip_val) and SAM (sharpness-aware minimisation), csrc/sam.hip.
"""
import contextlib
import math

import numpy as np
import torch
import torch.distributed as dist

from . import me as ME
from ._lib import call, call_on, load, ptr, require_gpu


class FlatParams:
    """Re-homes every parameter (and its .grad) of `model` into two contiguous fp32 buffers."""

    def __init__(self, model):
        self.params = [p for p in model.parameters() if p.requires_grad]
        total = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat = torch.empty(total, dtype=torch.float32, device=dev)
        self.grad = torch.zeros(total, dtype=torch.float32, device=dev)
        self.offsets = []
        self.generation = 0
        self.hooked = False
        self.buckets = None    # the GradientBuckets that reduce this buffer (data-parallel runs)
        off = 0
        for p in self.params:
            n = p.numel()
            self.flat[off:off + n].copy_(p.data.reshape(-1))
            p.data = self.flat[off:off + n].view(p.shape)
            p.grad = self.grad[off:off + n].view(p.shape)
            # lets backward kernels write this gradient in place (me._grad_out): (buffer, offset, owner)
            p._flat_ref = (self.grad, off, self)
            p._flat_taken = -1
            self.offsets.append(off)
            off += n
        self.total = total

    def zero_grad(self):
        """set_to_none semantics: backward kernels write fresh views of the flat buffer and autograd adopts them
        as .grad, so there is no `grad += new` pass; the buffer is cleared for parameters that get no gradient.
        A new generation starts: every parameter's slice may be handed out (once) again (me._grad_out)."""
        self.grad.zero_()
        self.generation += 1
        for p in self.params:
            p.grad = None

    def in_place(self, p, off):
        return p.grad is not None and p.grad.data_ptr() == self.grad.data_ptr() + 4 * off

    def gather_strays(self):
        """gradients that autograd produced outside the flat buffer (e.g. a bias gradient from a torch op) are
        copied in with one fused call; returns how many there were"""
        dst, src = [], []
        base = self.grad.data_ptr()
        for p, off in zip(self.params, self.offsets):
            g = p.grad
            if g is not None and g.data_ptr() != base + 4 * off:
                view = self.grad[off:off + p.numel()].view(p.shape)
                dst.append(view)
                src.append(p.grad)
                p.grad = view
        if dst:
            torch._foreach_copy_(dst, src)
        return len(dst)

    def broadcast(self, group=None, src=0):
        """DDP's start-up broadcast: every rank starts from rank `src`'s parameters"""
        dist.broadcast(self.flat, src=src, group=group)


class GradientBuckets:
    """Bucketed all-reduce (sum) of the flat gradient buffer, overlapped with backward.

    Parameters are registered in forward order, gradients arrive roughly in reverse, so buckets are
    contiguous slices walked from the END of the buffer.  xGMI is point-to-point (7 links per GPU):
    a few large messages (default 32 MiB) keep every link busy without paying per-message latency.

    A bucket is reduced as soon as its last gradient has been produced.  With the second backward stream active
    (me._WgradLane) the bucket's weight gradients may still be running there: the collective is issued from THAT
    stream (RCCL's stream then waits for the lane, which itself waits for everything queued on the main stream so far)
    and the main stream never waits before finish().
    RCCL executes the collectives of ONE communicator in issue order on one stream, so a bucket that still waits for
    the lane holds back the SyncBatchNorm statistics all-reduces issued after it -- by at most the lane's lag of about
    one layer.  `own_communicator=True` gives the buckets a communicator of their own (`dist.new_group`) and removes
    that coupling; it is not the default because two communicators in flight at once could not be exercised on more
    than one rank in this build's environment, and a same-communicator schedule is identical on every rank by
    construction.

    Uses per step: a model called on two sources before one backward pass (trainer_lighting_2d_multi.py:166-167) uses
    every parameter twice.  `set_uses(2)` (the two-source step objects) makes a bucket wait for 2 x its parameters: the
    trunk executor counts a parameter down once per backward pass over it (in C), autograd's post-accumulate hook fires
    once per parameter after every use has been summed and counts what the executor did not (`c_uses`)."""

    single_rank = False   # test hook: bucket and all-reduce even in a one-rank process group

    def __init__(self, flat, group=None, bucket_bytes=32 << 20, own_communicator=None, local=False):
        """`local=True`: no data parallelism for this optimiser even inside an initialised process group"""
        self.flat, self.group = flat, group
        self.world = dist.get_world_size(group) if (dist.is_initialized() and not local) else 1
        self.active = self.world > 1 or (self.single_rank and dist.is_initialized() and not local)
        self.handles = []
        self.index_of = {id(p): i for i, p in enumerate(flat.params)}
        self.bucket_of = {}
        self.pending0 = []
        self.slices = []
        self.issued_early = 0     # buckets reduced while backward was still being queued (hook or trunk executor)
        self.uses = 1             # uses of every parameter per step (set_uses)
        self.transport = None
        # LIDOG_DP_SAFE=1 (bench.py's fallback after a hung N > 1 run): no bucket leaves before backward has ended; finish()
        # reduces them one after the other on the compute stream through torch.distributed -- no bucket stream, no
        # second communicator in flight next to the statistics messages
        import os
        self.deferred = os.environ.get("LIDOG_DP_SAFE") == "1"
        if not self.active:
            return
        from .comm import transport
        self.transport = transport(group)
        if own_communicator and group is None:
            self.group = dist.new_group(ranks=list(range(dist.get_world_size())))
        cur_lo = cur_hi = flat.total
        count = 0
        members = []
        for p, off in reversed(list(zip(flat.params, flat.offsets))):
            members.append(p)
            cur_lo = off
            count += 1
            if (cur_hi - cur_lo) * 4 >= bucket_bytes:
                self._close(members, cur_lo, cur_hi, count)
                members, count, cur_hi = [], 0, cur_lo
        if members:
            self._close(members, cur_lo, cur_hi, count)
        # countdown per bucket, shared with the trunk executor (csrc/trunk.hip counts the trunk's parameters down in C
        # and reduces a bucket itself when it reaches 0): a host int32 array, not a list
        self.pending = np.array(self.pending0, dtype=np.int32)
        # per parameter: backward passes of this step that the trunk executor counted down in C
        self.c_uses = np.zeros(len(flat.params), dtype=np.int32)
        self.slice_table = np.array(self.slices, dtype=np.int64).reshape(-1, 2)
        for p in flat.params:
            p.register_post_accumulate_grad_hook(self._hook)
        flat.hooked = True     # parameters outside the trunk executor reach their bucket through these hooks
        flat.buckets = self

    def _close(self, members, lo, hi, count):
        b = len(self.slices)
        self.slices.append((lo, hi))
        self.pending0.append(count)
        for p in members:
            self.bucket_of[id(p)] = b

    def set_uses(self, uses):
        """how many times the model uses each parameter before one backward pass (1 or 2); call between steps"""
        if uses not in (1, 2):
            raise NotImplementedError(f"{uses} uses per step")
        if uses == self.uses:
            return
        self.uses = uses
        if self.active:
            self.pending[:] = np.array(self.pending0, dtype=np.int32) * uses
            self.c_uses[:] = 0

    def _hook(self, p):
        i = self.index_of[id(p)]
        off = self.flat.offsets[i]
        if not self.flat.in_place(p, off):   # stray gradient: bring it into the flat buffer before it is reduced
            view = self.flat.grad[off:off + p.numel()].view(p.shape)
            view.copy_(p.grad)
            p.grad = view
        b = self.bucket_of[id(p)]
        left = self.uses - int(self.c_uses[i])     # autograd summed every use it saw before this hook
        if left <= 0:
            return
        self.pending[b] -= left
        if self.pending[b] == 0:
            self.issued_early += 1
            self._reduce(b)

    def _reduce(self, b):
        if self.deferred:      # finish() reduces every bucket
            return
        lo, hi = self.slices[b]
        buf = self.flat.grad[lo:hi]
        lane = ME.wgrad_lane(buf.device) if buf.is_cuda else None
        tr = self.transport
        if tr.bucket_kind == "native":
            # on the bucket stream, behind what the compute stream and the weight-gradient stream hold now; nothing
            # waits for it before finish()
            tr.stream.wait_stream(torch.cuda.current_stream(buf.device))
            if lane is not None:
                tr.stream.wait_stream(lane.stream)
            call_on(tr.raw_stream, "lidog_allreduce_f32", ptr(buf), hi - lo, tr.comm_grad)
            return
        if lane is not None:
            main = torch.cuda.current_stream(buf.device)
            lane.stream.wait_stream(main)          # BatchNorm / bias gradients of the bucket are written on main
            with torch.cuda.stream(lane.stream):
                self.handles.append(dist.all_reduce(buf, group=self.group, async_op=True))
            return
        self.handles.append(dist.all_reduce(buf, group=self.group, async_op=True))

    def finish(self):
        """wait for every bucket; buckets whose hooks did not all fire (unused parameters) are reduced now"""
        if not self.active:
            return
        if self.deferred:
            # the caller (_FlatOptimizer._prepare) has joined the weight-gradient stream: every gradient is complete on
            # the current stream
            for lo, hi in self.slices:
                dist.all_reduce(self.flat.grad[lo:hi], group=self.group)
            self._reset()
            return
        for b, left in enumerate(self.pending.tolist()):
            if left > 0:
                self._reduce(b)
        for h in self.handles:
            h.wait()
        self.handles = []
        if self.transport.bucket_kind == "native":
            torch.cuda.current_stream(self.flat.grad.device).wait_stream(self.transport.stream)
        self._reset()

    def _reset(self):
        self.pending[:] = np.array(self.pending0, dtype=np.int32) * self.uses
        self.c_uses[:] = 0

    def executor_tables(self, params_by_slot):
        """int32 [n, 4] bucket of each (kernel, bias, BatchNorm weight, BatchNorm bias) of the trunk's convolutions,
        -1 where a convolution has no such parameter (lidog_trunk_backward, dp[9])"""
        out = np.full((len(params_by_slot), 4), -1, dtype=np.int32)
        for ci, slot in enumerate(params_by_slot):
            for j, p in enumerate(slot):
                if p is not None:
                    out[ci, j] = self.bucket_of[id(p)]
        return out


class TransposedKernels:
    """[K, Cout, Cin] copies of every sparse-convolution kernel [K, Cin, Cout] of the model (what the data gradients of
    the backward pass multiply by), refreshed by ONE launch after each optimiser step instead of one small transpose
    kernel per convolution inside the backward pass's dependent chain (63 launches per step).  A copy is used only
    while the parameter's version counter still has the value it had at the refresh: weights changed by anything
    else (load_state_dict, an in-place edit) fall back to the per-layer transpose (me._SparseConvFn.backward)."""

    def __init__(self, flat):
        self.flat = flat
        self.items = []
        desc, off, tiles = [], 0, 0
        for p, src in zip(flat.params, flat.offsets):
            if not getattr(p, "_lidog_sparse_kernel", False):
                continue
            shape = p.shape if p.dim() == 3 else (1,) + tuple(p.shape)
            K, Cin, Cout = shape
            desc.append((src, off, K, Cin, Cout, tiles))
            self.items.append((p, off, (K, Cout, Cin)))
            off += p.numel()
            tiles += K * (-(-Cin // 32)) * (-(-Cout // 32))
        self.total_tiles = tiles
        dev = flat.flat.device
        self.buf = torch.empty(off, dtype=torch.float32, device=dev)
        self.desc = torch.tensor(desc, dtype=torch.int64, device=dev).view(-1, 6) if desc else None
        self.generation = 0     # refreshes so far (precision.Bf16Training packs from these copies and compares)
        for p, o, shape in self.items:
            p._wt_view = self.buf[o:o + p.numel()].view(shape)
            p._wt_version = -1
            p._wt_owner = self
        self.refresh()

    def refresh(self):
        self.generation += 1
        if not self.items or not self.buf.is_cuda:
            return
        call("lidog_transpose_batched", ptr(self.flat.flat), ptr(self.buf), ptr(self.desc), len(self.items),
             self.total_tiles)
        for p, _, _ in self.items:
            p._wt_version = p._version


class _FlatOptimizer:
    """Common part of the fused optimisers: flat buffers, gradient buckets, and torch's rule that a parameter
    WITHOUT a gradient is skipped entirely (no weight decay, no moment decay, no step count) -- e.g. `final.*`
    while `epoch < warmup_epochs` (trainer_lighting_2d.py:193-201)."""

    def __init__(self, model, lr, group=None, bucket_bytes=32 << 20, local=False):
        self.flat = FlatParams(model)
        self.lr = float(lr)
        self.base_lr = float(lr)
        self.param_steps = [0] * len(self.flat.params)   # torch keeps `step` per parameter
        self.buckets = GradientBuckets(self.flat, group, bucket_bytes, local=local)
        if self.buckets.world > 1:
            self.flat.broadcast(group)     # DDP's start-up broadcast of rank 0's parameters
        self.strays = 0
        self._strays_early = 0
        self.transposed = TransposedKernels(self.flat)
        self.sqnorm = None    # device double: the squared gradient norm of the last grad_norm / clip_grad_norm
        self._sqnorm_ws = None

    @property
    def steps(self):
        return max(self.param_steps) if self.param_steps else 0

    def zero_grad(self):
        self.flat.zero_grad()

    def _runs(self):
        """contiguous [lo, hi) element ranges of parameters that received a gradient, with their (common) new step
        count: one range covering everything in the usual case"""
        runs = []
        params, offs = self.flat.params, self.flat.offsets
        for i, (p, off) in enumerate(zip(params, offs)):
            if p.grad is None:
                continue
            self.param_steps[i] += 1
            st, hi = self.param_steps[i], off + p.numel()
            if runs and runs[-1][1] == off and runs[-1][2] == st:
                runs[-1][1] = hi
            else:
                runs.append([off, hi, st])
        return runs

    def _prepare(self):
        lane = ME.wgrad_lane(self.flat.grad.device) if self.flat.grad.is_cuda else None
        if lane is not None:   # normally joined already by the engine callback at the end of backward()
            lane.join()
        self.strays = self.flat.gather_strays() + self._strays_early   # those a norm taken before this step gathered
        self._strays_early = 0
        self.buckets.finish()
        return 1.0 / self.buckets.world

    # ---- the global gradient norm (csrc/sam.hip)
    def _complete_gradients(self):
        """what step() does before its kernel -- the weight-gradient lane joined, stray gradients gathered, the buckets
        finished -- without counting a step: the whole gradient is in the flat buffer, on the current stream.  step()
        repeats it and finds nothing left to do; `strays` keeps this call's count.  Returns the gradient scale."""
        scale = self._prepare()
        self._strays_early = self.strays
        return scale

    def _launch_sqnorm(self, out, adaptive=False):
        """out[0] (a device double) = sum (t g)^2 over the flat gradient, t = |w| if `adaptive` else 1: two launches, a
        fixed summation order, nothing read back"""
        f = self.flat
        require_gpu(f.grad, "the gradients of the norm's optimiser")
        if self._sqnorm_ws is None:
            self._sqnorm_ws = torch.empty(load().lidog_flat_sqnorm_ws(f.total) // 8, dtype=torch.float64,
                                          device=f.grad.device)
        call("lidog_flat_sqnorm", ptr(f.grad), ptr(f.flat) if adaptive else None, f.total,
             SQNORM_ADAPTIVE if adaptive else SQNORM_PLAIN, ptr(self._sqnorm_ws), ptr(out))

    def _own_sqnorm(self):
        if self.sqnorm is None:
            self.sqnorm = torch.zeros(1, dtype=torch.float64, device=self.flat.grad.device)
        return self.sqnorm

    def grad_norm(self):
        """the 2-norm of the whole gradient as a 0-dim float64 tensor on the device (torch's `total_norm`), taken now:
        call it between backward() and step().  The host is not synchronised; `.item()` is the caller's to pay."""
        check_single_rank("grad_norm()")
        scale = self._complete_gradients()
        self._launch_sqnorm(self._own_sqnorm())
        return (self.sqnorm.sqrt() * scale).reshape(())

    def clip_grad_norm(self, max_norm):
        """torch.nn.utils.clip_grad_norm_(parameters, max_norm) on the flat gradient, between backward() and step(): the
        norm (two launches) and ONE scaling launch that reads it on the device (include/lidog_amd.h:lidog_flat_clip).
        The squared norm from before the clipping stays in `self.sqnorm`."""
        check_clip_argument(max_norm)
        check_single_rank("clip_grad_norm()")
        scale = self._complete_gradients()
        self._launch_sqnorm(self._own_sqnorm())
        call("lidog_flat_clip", ptr(self.flat.grad), self.flat.total, ptr(self.sqnorm), float(max_norm), float(scale))

    def state_dict(self):
        sd = {"lr": self.lr, "base_lr": self.base_lr, "param_steps": list(self.param_steps), "kind": type(self).__name__}
        sd.update({k: getattr(self, k) for k in self._state})
        return sd

    def torch_state_dict(self):
        """the state in torch.optim's layout -- `state` {index: {step, per-parameter tensors}} + `param_groups` with the
        parameters numbered in model.parameters() order -- i.e. what Lightning stores as `optimizer_states[0]` and what
        the reference's `trainer.fit(ckpt_path=...)` (train_lidog.py:298-301) hands to torch.optim.Adam / SGD
        .load_state_dict.  Parameters that never received a gradient have no entry, as in torch."""
        state = {}
        for i, (p, off) in enumerate(zip(self.flat.params, self.flat.offsets)):
            if self.param_steps[i] == 0:
                continue
            entry = {k: getattr(self, k)[off:off + p.numel()].view(p.shape).detach().clone() for k in self._state}
            if "exp_avg" in entry:
                entry["step"] = torch.tensor(float(self.param_steps[i]))
            state[i] = entry
        group = dict(self._torch_group(), lr=self.lr, initial_lr=self.base_lr, params=list(range(len(self.flat.params))))
        return {"state": state, "param_groups": [group]}

    def _load_torch_layout(self, sd):
        """inverse of torch_state_dict: a checkpoint written by the reference (torch.optim state through Lightning)"""
        groups = sd["param_groups"]
        order = [i for g in groups for i in g["params"]]
        if len(order) != len(self.flat.params):
            raise ValueError(f"optimizer state for {len(order)} parameters, the model has {len(self.flat.params)}")
        for k in self._state:
            getattr(self, k).zero_()
        self.param_steps = [0] * len(self.flat.params)
        for pos, idx in enumerate(order):
            entry = sd["state"].get(idx)
            if entry is None:
                continue
            p, off = self.flat.params[pos], self.flat.offsets[pos]
            for k in self._state:
                if entry.get(k) is not None:
                    getattr(self, k)[off:off + p.numel()].copy_(entry[k].reshape(-1).to(getattr(self, k).device))
            step = entry.get("step", 1)
            self.param_steps[pos] = int(step.item() if torch.is_tensor(step) else step)
        self.lr = float(groups[0]["lr"])
        self.base_lr = float(groups[0].get("initial_lr", groups[0]["lr"]))
        self.transposed.refresh()

    def load_state_dict(self, sd):
        if "state" in sd and "param_groups" in sd:     # torch.optim layout (a checkpoint of the reference / Lightning)
            return self._load_torch_layout(sd)
        for k in self._state:
            getattr(self, k).copy_(sd[k].to(getattr(self, k).device))
        self.lr, self.base_lr = float(sd["lr"]), float(sd.get("base_lr", sd["lr"]))
        if "param_steps" in sd:
            self.param_steps = list(sd["param_steps"])
        else:   # round-1 checkpoints stored one global step count
            self.param_steps = [int(sd["steps"])] * len(self.flat.params)
        self.transposed.refresh()   # the model's weights were (re)loaded before this call


class FlatAdam(_FlatOptimizer):
    """torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8, weight_decay) semantics, one fused HIP kernel
    over the flat buffer (csrc/optim.hip:k_adam); `grad_scale` folds the 1/world_size of DDP averaging."""
    _state = ("exp_avg", "exp_avg_sq")

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, group=None,
                 bucket_bytes=32 << 20, local=False):
        super().__init__(model, lr, group, bucket_bytes, local)
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.exp_avg = torch.zeros_like(self.flat.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat.flat)

    def _torch_group(self):
        return {"betas": tuple(self.betas), "eps": self.eps, "weight_decay": self.weight_decay, "amsgrad": False,
                "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None}

    def step(self):
        scale = self._prepare()
        f = self.flat
        for lo, hi, st in self._runs():
            call("lidog_adam_step", ptr(f.flat[lo:hi]), ptr(f.grad[lo:hi]), ptr(self.exp_avg[lo:hi]),
                 ptr(self.exp_avg_sq[lo:hi]), hi - lo, float(self.lr), float(self.betas[0]), float(self.betas[1]),
                 float(self.eps), float(self.weight_decay), st, float(scale))
        self.transposed.refresh()


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, weight_decay, nesterov=True) semantics (trainer_lighting_2d.py:351-355 with
    momentum 0.98, :26), one fused HIP kernel over the flat buffer (csrc/optim.hip:k_sgd)."""
    _state = ("momentum_buffer",)

    def __init__(self, model, lr=1e-3, momentum=0.98, weight_decay=0.0, nesterov=True, group=None,
                 bucket_bytes=32 << 20, local=False):
        super().__init__(model, lr, group, bucket_bytes, local)
        if nesterov and momentum <= 0:
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")   # torch's own check
        self.momentum, self.weight_decay, self.nesterov = momentum, weight_decay, nesterov
        self.momentum_buffer = torch.zeros_like(self.flat.flat)

    def _torch_group(self):
        return {"momentum": self.momentum, "dampening": 0, "weight_decay": self.weight_decay, "nesterov": self.nesterov,
                "maximize": False, "foreach": None, "differentiable": False, "fused": None}

    def step(self):
        scale = self._prepare()
        f = self.flat
        for lo, hi, _ in self._runs():
            call("lidog_sgd_step", ptr(f.flat[lo:hi]), ptr(f.grad[lo:hi]), ptr(self.momentum_buffer[lo:hi]), hi - lo,
                 float(self.lr), float(self.momentum), float(self.weight_decay), 1 if self.nesterov else 0,
                 float(scale))
        self.transposed.refresh()


def make_optimizer(name, model, lr, weight_decay=1e-4, momentum=0.98, group=None):
    """optimizer_name of the reference's pipelines: 'Adam' | 'SGD' (anything else raises, as the reference does)"""
    if name == "Adam":
        return FlatAdam(model, lr=lr, weight_decay=weight_decay, group=group)
    if name == "SGD":
        return FlatSGD(model, lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=True, group=group)
    raise NotImplementedError(name)


# ------------------------------------------------------------------ weight averaging (csrc/wavg.hip)
WAVG_COPY, WAVG_EMA, WAVG_SWA, WAVG_SWAP = range(4)     # LIDOG_WAVG_* of include/lidog_amd.h
WAVG_BLOCK_ELEMS = 1024      # what one workgroup covers per sweep: 256 threads, one float4 each
WAVG_MAX_BLOCKS = 2048       # a memory-bound pass: about 8 workgroups per CU, the rest is grid-strided


def wavg_table(triples, max_blocks=WAVG_MAX_BLOCKS):
    """(int64 numpy table, workgroups) of lidog_wavg_apply over `triples` [(live address, average address, elements)]:
    the triples, then block0 [n + 1], the first workgroup of every segment.  A segment gets workgroups in proportion to
    its share of all elements, at least one and no more than it has sweeps for; an empty one gets none.  The entry point
    cannot read a table that lives on the device, so everything it relies on is checked HERE: counts, alignment, and
    that no two of the 2 n address ranges overlap."""
    triples = [tuple(int(v) for v in t) for t in triples]
    spans = []
    for s, (live, avg, n) in enumerate(triples):
        if n < 0:
            raise ValueError(f"wavg_table: segment {s} has {n} elements")
        if n == 0:
            continue
        if live <= 0 or avg <= 0 or live % 4 or avg % 4:
            raise ValueError(f"wavg_table: segment {s}: addresses {live:#x}, {avg:#x} are not those of float32 arrays")
        spans += [(live, live + 4 * n, s), (avg, avg + 4 * n, s)]
    spans.sort()
    for (_, hi, s0), (lo, _, s1) in zip(spans, spans[1:]):
        if lo < hi:
            raise ValueError(f"wavg_table: the ranges of segments {s0} and {s1} overlap")
    total = sum(n for _, _, n in triples)
    block0 = [0]
    for _, _, n in triples:
        nb = min(-(-n // WAVG_BLOCK_ELEMS), max(1, n * max_blocks // total)) if n else 0
        block0.append(block0[-1] + nb)
    table = np.array([v for t in triples for v in t] + block0, dtype=np.int64)
    return table, block0[-1]


class WeightAverage:
    """The average of a model's weights along its training trajectory, kept next to the live weights and updated by
    ONE launch per step (csrc/wavg.hip) over the optimiser's flat parameter buffer and every floating-point buffer of
    the model (the BatchNorm running statistics; integer buffers -- num_batches_tracked -- are not averaged).

    mode "ema": a = tau a + (1 - tau) p, the reference's MomentumUpdater (utils/common/momentum.py) with its cosine
                schedule tau_s = final - (final - decay) (cos(pi s / total_steps) + 1) / 2 over the updates made so far;
                `final_decay=None`: tau = decay throughout.
    mode "swa": a = a + (p - a) / (n + 1) after n updates, torch.optim.swa_utils.AveragedModel's default.
    The first update copies.  Every rank of a data-parallel run averages its own (identical) weights: no collective.

        avg = WeightAverage(opt, model, "ema", decay=0.996)
        ...; opt.step(); avg.update()
        with avg.applied():                      # the model computes with the averaged weights and statistics, in place
            validate(model)
        sd = avg.averaged_state_dict()           # CPU clones under the model's own keys; no swap

    applied() exchanges live and averaged values behind autograd's back (no version counter moves), so on entry and on
    exit it refreshes the optimiser's transposed kernels -- which also advances their generation, the signal the bf16
    training table re-packs on.  Enter it OUTSIDE precision.scope: a bf16 evaluation packs when its scope opens."""
    MODES = ("ema", "swa")

    @staticmethod
    def check_arguments(mode, decay=0.996, final_decay=None, total_steps=None):
        if mode not in WeightAverage.MODES:
            raise ValueError(f"weight average mode {mode!r} (one of {WeightAverage.MODES})")
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f"decay {decay}: it lies in [0, 1]")
        if final_decay is not None:
            if not decay <= final_decay <= 1.0:
                raise ValueError(f"final_decay {final_decay}: decay ({decay}) <= final_decay <= 1")
            if mode == "ema" and (total_steps is None or int(total_steps) <= 0):
                raise ValueError("a cosine schedule of the decay (final_decay) needs total_steps > 0")

    def __init__(self, optimizer, model, mode="ema", decay=0.996, final_decay=None, total_steps=None):
        self.check_arguments(mode, decay, final_decay, total_steps)
        self.mode, self.decay = mode, float(decay)
        self.final_decay = None if final_decay is None else float(final_decay)
        self.total_steps = None if total_steps is None else int(total_steps)
        self.num_updates = 0
        self.optimizer, self.model = optimizer, model
        self._applied = False
        flat = optimizer.flat
        require_gpu(flat.flat, "the parameters of WeightAverage's optimiser")
        self.params = torch.zeros_like(flat.flat)
        owned = {id(p) for p in flat.params}
        stray = [k for k, p in model.named_parameters() if id(p) not in owned]
        if stray:
            raise ValueError(f"WeightAverage: {stray[:3]} ... are not parameters of the optimiser's flat buffer")
        # the live buffers are held: their memory outlives the table that names it
        persistent = set(model.state_dict(keep_vars=True))
        self._live = [(k, b) for k, b in model.named_buffers() if k in persistent and b.is_floating_point()]
        offs, off = [], 0
        for k, b in self._live:
            if b.dtype != torch.float32 or not b.is_contiguous() or b.device != flat.flat.device:
                raise ValueError(f"WeightAverage: buffer {k} must be contiguous float32 on the parameters' device")
            offs.append(off)
            off += -(-b.numel() // 4) * 4         # every slice starts on a 16-byte boundary, as torch's allocations do
        self.buffers = torch.zeros(off, dtype=torch.float32, device=flat.flat.device)
        self._buffer_views = [self.buffers[o:o + b.numel()].view(b.shape) for o, (_, b) in zip(offs, self._live)]
        triples = [(flat.flat.data_ptr(), self.params.data_ptr(), flat.total)]
        triples += [(b.data_ptr(), v.data_ptr(), b.numel()) for (_, b), v in zip(self._live, self._buffer_views)]
        table, self.n_blocks = wavg_table(triples)
        self.n_segs = len(triples)
        self._addresses = [t[0] for t in triples]
        self.table = torch.from_numpy(table).to(flat.flat.device)

    # ------------------------------------------------------------------ the schedule
    def tau(self, s):
        """the decay of the update after `s` earlier ones (update_tau of the reference, in python doubles)"""
        if self.final_decay is None:
            return self.decay
        s = min(s, self.total_steps)
        return self.final_decay - (self.final_decay - self.decay) * (math.cos(math.pi * s / self.total_steps) + 1) / 2

    def coefficients(self, s):
        """(kernel mode, c0, c1) of the update after `s` earlier ones"""
        if s == 0:
            return WAVG_COPY, 0.0, 0.0
        if self.mode == "ema":
            tau = self.tau(s)
            return WAVG_EMA, float(tau), float(1.0 - tau)
        return WAVG_SWA, float(s + 1), 0.0

    # ------------------------------------------------------------------ launches
    def _check_live(self):
        now = [self.optimizer.flat.flat.data_ptr()] + [b.data_ptr() for _, b in self._live]
        named = dict(self.model.named_buffers())
        if now != self._addresses or any(named.get(k) is not b for k, b in self._live):
            raise RuntimeError("WeightAverage: the model's parameters or buffers moved in memory since it was built "
                               "(.to(), a new optimiser, a re-registered buffer): build a new WeightAverage")

    def _launch(self, mode, c0=0.0, c1=0.0):
        with torch.cuda.device(self.table.device):
            call("lidog_wavg_apply", ptr(self.table), self.n_segs, self.n_blocks, mode, c0, c1)

    def update(self):
        """fold the live weights into the average: call after optimizer.step().  One launch."""
        if self._applied:
            raise RuntimeError("WeightAverage.update() inside applied(): the live weights are swapped out")
        if self.optimizer.flat.flat.data_ptr() != self._addresses[0]:
            self._check_live()
        self._launch(*self.coefficients(self.num_updates))
        self.num_updates += 1

    @contextlib.contextmanager
    def applied(self):
        """inside, the model holds the averaged parameters and running statistics and `self` holds the live ones; on
        exit every live byte is back.  One SWAP launch each way, and the per-parameter caches are made consistent."""
        if self._applied:
            raise RuntimeError("WeightAverage.applied() cannot be nested")
        if self.num_updates == 0:
            raise RuntimeError("WeightAverage.applied() before the first update(): there is no average yet")
        self._check_live()
        self._applied = True
        self._swap()
        try:
            yield self
        finally:
            self._swap()
            self._applied = False

    def _swap(self):
        self._launch(WAVG_SWAP)
        self.optimizer.transposed.refresh()     # the copies follow the weights; bf16 tables compare its generation

    # ------------------------------------------------------------------ state
    def averaged_state_dict(self):
        """the averaged model under the model's own state-dict keys, as CPU clones: averaged parameters and floating-point
        buffers, the live values of everything else (the integer counters, brought up to date by the state-dict hooks)"""
        self._check_live()
        live = self.model.state_dict()
        flat = self.optimizer.flat
        out = {k: v.detach().cpu().clone() for k, v in live.items()}
        if self._applied:                       # the exchange is in force: the average sits in the live storage
            return out
        index = {id(p): off for p, off in zip(flat.params, flat.offsets)}
        for k, p in self.model.named_parameters():
            if k in out:
                off = index[id(p)]
                out[k] = self.params[off:off + p.numel()].view(p.shape).cpu().clone()
        for (k, _), v in zip(self._live, self._buffer_views):
            out[k] = v.cpu().clone()
        return out

    def load_averaged_state_dict(self, sd):
        """inverse of averaged_state_dict (a checkpoint's `averaged_state_dict` without its `model.` prefix)"""
        if self._applied:
            raise RuntimeError("WeightAverage.load_averaged_state_dict() inside applied()")
        flat = self.optimizer.flat
        index = {id(p): off for p, off in zip(flat.params, flat.offsets)}
        for k, p in self.model.named_parameters():
            off = index[id(p)]
            self.params[off:off + p.numel()].copy_(sd[k].reshape(-1).to(self.params.device, torch.float32))
        for (k, _), v in zip(self._live, self._buffer_views):
            v.copy_(sd[k].to(v.device, torch.float32))

    def state_dict(self):
        return {"mode": self.mode, "decay": self.decay, "final_decay": self.final_decay,
                "total_steps": self.total_steps, "num_updates": self.num_updates}

    def load_state_dict(self, sd):
        self.check_arguments(sd["mode"], sd["decay"], sd["final_decay"], sd["total_steps"])
        self.mode, self.decay, self.final_decay = sd["mode"], float(sd["decay"]), sd["final_decay"]
        self.total_steps, self.num_updates = sd["total_steps"], int(sd["num_updates"])

    # ------------------------------------------------------------------ SWA's BatchNorm pass
    def update_bn(self, batches, forward):
        """re-estimate the running statistics of the AVERAGED model (torch.optim.swa_utils.update_bn): inside applied(),
        zero mean / unit variance, every BatchNorm's momentum None (the cumulative average, me._training_momentum),
        `forward(batch)` in training mode without autograd over `batches`; then momenta, counters and mode return.  The
        live statistics are untouched: the exit swap carries the new ones into the average's storage."""
        bns = [m for m in self.model.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)
               and m.track_running_stats and m.running_mean is not None]
        if not bns:
            return
        with self.applied():
            was_training = self.model.training
            saved = []
            for bn in bns:
                ME._flush_batch_counter(bn)
                saved.append((bn.momentum, bn.num_batches_tracked.clone(), bn.training))
                bn.running_mean.zero_()
                bn.running_var.fill_(1.0)
                bn.num_batches_tracked.zero_()
                bn.momentum = None
            try:
                self.model.train()
                with torch.no_grad():
                    for batch in batches:
                        forward(batch)
            finally:
                for bn, (momentum, count, _) in zip(bns, saved):
                    ME._flush_batch_counter(bn)
                    bn.momentum = momentum
                    bn.num_batches_tracked.copy_(count)
                self.model.train(was_training)
                for bn, (_, _, training) in zip(bns, saved):
                    bn.training = training


# ------------------------------------------------------------------ gradient norm, clipping, SAM (csrc/sam.hip)
SQNORM_PLAIN, SQNORM_ADAPTIVE = 0, 1     # LIDOG_SQNORM_* of include/lidog_amd.h
FLAT_MAX_BLOCKS = 2048                   # LIDOG_FLAT_MAX_BLOCKS: workgroups of 1024 elements per sweep


def check_single_rank(what):
    """the global gradient norm is taken over one rank's flat buffer; where it stands relative to the bucket
    all-reduces of a data-parallel run has not been verified on more than one GPU"""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f"{what} with {dist.get_world_size()} ranks: sharpness-aware minimisation and "
                                  "gradient clipping are one-rank features (the norm is not reduced across ranks)")


def check_clip_argument(max_norm):
    if not (isinstance(max_norm, (int, float)) and max_norm > 0):      # a NaN fails the comparison
        raise ValueError(f"grad_clip_norm {max_norm}: the largest gradient norm is positive")


def check_sam_arguments(sam_rho=None, sam_adaptive=False, grad_clip_norm=None):
    """the checks of build_step / Fit / the command line for sam_rho, sam_adaptive and grad_clip_norm"""
    if sam_rho is not None:
        SAM.check_arguments(sam_rho, sam_adaptive)
    elif sam_adaptive:
        raise ValueError("sam_adaptive goes with sam_rho: the adaptive form scales SAM's neighbourhood")
    if grad_clip_norm is not None:
        check_clip_argument(grad_clip_norm)


class SAM:
    """Sharpness-aware minimisation (Foret et al., ICLR 2021) around a FlatAdam / FlatSGD: the gradient that the
    optimiser steps along is taken at w + e, the worst point of a rho-neighbourhood of the weights to first order,

        e = rho g / ||g||                                  adaptive (ASAM, Kwon et al.): e = rho w^2 g / || |w| g ||

        loss(model(batch)).backward();  sam.first_step()        # w -> w + e, the weights saved
        opt.zero_grad(); loss(model(batch)).backward()          # the same batch, BatchNorm statistics frozen
        sam.second_step();  opt.step()                          # w back, bit for bit; the step uses the new gradient

    first_step is the norm (two launches, a device double) and ONE launch over the flat buffers that saves and moves
    the weights (include/lidog_amd.h:lidog_sam_perturb); second_step is a device copy of the saved weights.  Both end
    with TransposedKernels.refresh(): the [K, Cout, Cin] copies follow the weights and the generation that bf16 tables
    compare advances (a precision="bf16" step re-packs after each, trainer._Step).  Parameters without a gradient are
    not moved.  No state: nothing goes into a checkpoint.  One rank."""

    @staticmethod
    def check_arguments(rho, adaptive=False):
        if not (isinstance(rho, (int, float)) and rho > 0 and math.isfinite(rho)):
            raise ValueError(f"sam_rho {rho}: the neighbourhood's radius is positive and finite")

    def __init__(self, optimizer, rho=0.05, adaptive=False):
        self.check_arguments(rho, adaptive)
        check_single_rank("SAM")
        if optimizer.buckets.world > 1:
            raise NotImplementedError(f"SAM over a data-parallel optimiser ({optimizer.buckets.world} ranks)")
        self.optimizer, self.rho, self.adaptive = optimizer, float(rho), bool(adaptive)
        flat = optimizer.flat
        require_gpu(flat.flat, "the parameters of SAM's optimiser")
        self.backup = torch.empty_like(flat.flat)       # allocated once
        self.sqnorm = torch.zeros(1, dtype=torch.float64, device=flat.flat.device)   # of the last first_step
        self.perturbed = False

    def first_step(self):
        """after backward(): w -> w + e from the gradient in the flat buffer; no optimiser step is counted"""
        if self.perturbed:
            raise RuntimeError("SAM.first_step() twice: second_step() restores the weights first")
        opt, f = self.optimizer, self.optimizer.flat
        opt._complete_gradients()      # the weight-gradient lane is joined: no gradient is still being written
        opt._strays_early = 0           # this pass's gradient is thrown away; step() reports the second pass's strays
        opt._launch_sqnorm(self.sqnorm, self.adaptive)
        call("lidog_sam_perturb", ptr(f.flat), ptr(f.grad), ptr(self.backup), f.total, ptr(self.sqnorm), self.rho,
             1 if self.adaptive else 0)
        self.perturbed = True
        opt.transposed.refresh()

    def second_step(self):
        """after the second backward(): every byte of the weights is back (a copy, never w - e); then optimizer.step()"""
        if not self.perturbed:
            raise RuntimeError("SAM.second_step() without first_step()")
        self.optimizer.flat.flat.copy_(self.backup)
        self.perturbed = False
        self.optimizer.transposed.refresh()

    def grad_norm(self):
        """the norm first_step divided by (|| g ||, adaptive: || |w| g ||), a 0-dim float64 tensor on the device"""
        return self.sqnorm.sqrt().reshape(())


# ------------------------------------------------------------------ learning-rate schedules (stepped per epoch)
class _Scheduler:
    """torch.optim.lr_scheduler semantics for ONE parameter group: construction performs the initial step
    (last_epoch 0), `step()` advances one epoch and writes optimizer.lr.  Same recurrences in python doubles as
    torch's `get_lr`, so the sequence is identical (tests/test_optim_cpu.py compares with torch itself)."""

    def __init__(self, optimizer):
        self.optimizer = optimizer
        self.base_lr = optimizer.base_lr
        self.last_epoch = 0
        optimizer.lr = self._lr(optimizer.lr)

    def step(self):
        self.last_epoch += 1
        self.optimizer.lr = self._lr(self.optimizer.lr)
        return self.optimizer.lr

    def state_dict(self):
        # last_epoch / base_lrs / _last_lr are the keys of torch's schedulers (what Lightning stores and restores)
        return {"last_epoch": self.last_epoch, "base_lr": self.base_lr, "base_lrs": [self.base_lr],
                "_last_lr": [self.optimizer.lr], "kind": type(self).__name__}

    def load_state_dict(self, sd):
        self.last_epoch = int(sd["last_epoch"])
        self.base_lr = float(sd["base_lr"] if "base_lr" in sd else sd["base_lrs"][0])


class CosineAnnealingLR(_Scheduler):
    def __init__(self, optimizer, T_max=10, eta_min=0.0):
        self.T_max, self.eta_min = T_max, eta_min
        super().__init__(optimizer)

    def _lr(self, lr):
        t, T, lo = self.last_epoch, self.T_max, self.eta_min
        if t == 0:
            return lr
        if (t - 1 - T) % (2 * T) == 0:
            return lr + (self.base_lr - lo) * (1 - math.cos(math.pi / T)) / 2
        return (1 + math.cos(math.pi * t / T)) / (1 + math.cos(math.pi * (t - 1) / T)) * (lr - lo) + lo


class ExponentialLR(_Scheduler):
    def __init__(self, optimizer, gamma=0.99):
        self.gamma = gamma
        super().__init__(optimizer)

    def _lr(self, lr):
        return lr if self.last_epoch == 0 else lr * self.gamma


class CyclicLR(_Scheduler):
    """mode 'triangular2' (scale 1 / 2^(cycle-1) per cycle), cycle_momentum=False"""

    def __init__(self, optimizer, base_lr, max_lr, step_size_up=5, step_size_down=None):
        up = float(step_size_up)
        down = float(step_size_down) if step_size_down is not None else up
        self.total_size = up + down
        self.step_ratio = up / self.total_size
        self.cyc_base, self.cyc_max = float(base_lr), float(max_lr)
        super().__init__(optimizer)

    def _lr(self, lr):
        cycle = math.floor(1 + self.last_epoch / self.total_size)
        x = 1.0 + self.last_epoch / self.total_size - cycle
        scale = x / self.step_ratio if x <= self.step_ratio else (x - 1) / (self.step_ratio - 1)
        height = (self.cyc_max - self.cyc_base) * scale
        return self.cyc_base + height * (1.0 / (2.0 ** (cycle - 1)))


def make_scheduler(name, optimizer):
    """scheduler_name of the reference's pipelines with the reference's hyper-parameters
    (trainer_lighting_2d.py:379-389); None -> no schedule"""
    if name is None:
        return None
    if name == "CosineAnnealingLR":
        return CosineAnnealingLR(optimizer, T_max=10)
    if name == "ExponentialLR":
        return ExponentialLR(optimizer, gamma=0.99)
    if name == "CyclicLR":
        return CyclicLR(optimizer, base_lr=optimizer.base_lr / 10000, max_lr=optimizer.base_lr, step_size_up=5)
    raise NotImplementedError(name)


def shard_indices(n, rank, world, shuffle=False, seed=0, epoch=0, drop_last=False):
    """torch.utils.data.DistributedSampler semantics (what Lightning injects under strategy='ddp'): optional
    permutation seeded with seed + epoch, padded by wrap-around to a multiple of `world` (so every rank gets the
    same number of samples and no rank runs out of SyncBatchNorm partners), rank-strided."""
    if shuffle:
        g = torch.Generator()
        g.manual_seed(seed + epoch)
        idx = torch.randperm(n, generator=g).tolist()
    else:
        idx = list(range(n))
    if drop_last and n % world:
        total = (n // world) * world
        idx = idx[:total]
    else:
        total = -(-n // world) * world
        pad = total - len(idx)
        if pad > 0 and idx:
            idx += (idx * -(-pad // len(idx)))[:pad]
    return idx[rank:total:world]
