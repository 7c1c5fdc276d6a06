"""Training step of LiDOG on the GPU: loss composition, Adam on a flat HBM buffer, RCCL data parallelism.

Restates what the reference gets from pytorch-lightning (not installable here, and python that the GPU
box never receives):
  training_step        utils/pipelines/trainer_lighting_2d.py:141-201  (PLTTrainer2D)
                       utils/pipelines/trainer_lighting.py:92-104      (PLTTrainer, source-only)
                       utils/pipelines/trainer_lighting_robustnet.py    (PLTRobustNet, one source)
  two sources          utils/pipelines/trainer_lighting_2d_multi.py:135-215 (PLTTrainer2DMulti), trainer_lighting.py:92-116,
                       trainer_lighting_robustnet.py:96-150: the step classes below with num_sources=2
  configure_optimizers utils/pipelines/trainer_lighting_2d.py:349-394  (Adam lr, weight_decay 1e-4)
  DDP + SyncBN         train_lidog.py:227-231,286-289                   (strategy='ddp')

One process per GPU; gradients live in ONE contiguous fp32 buffer that is all-reduced over RCCL in
a few large buckets launched as soon as their last gradient is produced (overlapping the rest of
backward), then consumed by a single fused Adam kernel.
"""
import contextlib as _contextlib
import os as _os

import torch
import torch.distributed as dist

from . import me as ME
from . import optim as _optim
from . import precision as _precision
from .losses import iw_loss, make_aux_criterion, make_bev_criterion, make_criterion
from .optim import (FlatAdam, FlatParams, FlatSGD, GradientBuckets, make_optimizer, make_scheduler,  # noqa: F401
                    shard_indices)


class _Step:
    """What every step shares.  With `num_sources=2` a batch carries a second source (`source_*1`, `coords_int1`): the
    model runs on source 0, then on source 1 (BatchNorm statistics move twice), then ONE backward pass and one step;
    the gradient buckets wait for both uses of every parameter (GradientBuckets.set_uses).
    `training_step(batch, prefetch=next_batch)` builds the next batch's coordinate maps on a side stream while the GPU
    still works on this step, from the trace of map uses recorded by the first forward pass: the data-loader-side half
    of the reference's step (ME builds its maps inside the forward call) moved off the critical path, not skipped.
    Subclasses define `_losses(batch, epoch) -> (total, {name: loss}, [semantic output of each source])`.
    `metrics`: a lidog_amd.metrics.StepMetrics, or None (the default).  When set, training_step hands it the logits and
    labels of every source (LiDOGStep: and of every BEV level) and the step's losses; the step computes and returns
    what it does without.
    `precision`: None / "fp32" (the fp32 step) or "bf16": the eligible sparse convolutions run forward, data gradient
    and weight gradient on the bf16 matrix instruction (lidog_amd.precision; fp32 master weights, gradients and optimiser
    state), the step leaves the trunk executor for the operator path, and the packed operand tables (`bf16`, a
    precision.Bf16Training) are refreshed after every optimiser step.  `precision_ctx`: the context of the last bf16
    step (its `.launches` count the routes).  One rank only.
    `sem_criterion`: the point loss by name, losses.sem_criterion of the reference's configurations
    (losses.make_criterion: CELoss, DICELoss, SoftDICELoss, FocalLoss); `num_classes` = 19 gives SoftDICELoss the KITTI
    soft labels.
    `sem_aux_criterion`: None, or an auxiliary point loss by name (losses.make_aux_criterion: LovaszSoftmaxLoss) that is
    added to the point loss of every source, times `sem_aux_weight`: the step's `sem_loss` (`sem_loss0` / `sem_loss1`) is
    that sum, so the loss dictionaries and the logged keys keep their shape.  None launches nothing.
    `sam`: None, or an optim.SAM over the step's optimiser: every training step takes its gradient at the perturbed
    weights, at the cost of a second forward and backward pass over the batch (_sam_second_pass); losses and metrics are
    the first pass's, at the live weights.  `grad_clip_norm`: None, or the largest 2-norm of the whole gradient
    (torch's clip_grad_norm_, Lightning's gradient_clip_val): the norm and one scaling launch between backward and the
    optimiser step; with `sam` it is the second pass's gradient that is clipped.  Both: one rank only; None launches
    nothing."""

    metrics = None
    bf16 = None                         # the packed tables of precision="bf16"
    precision_ctx = None
    metric_losses = ("sem_loss",)       # the loss names of one source, in the order of the step's loss dict
    metric_bev = False                  # the BEV levels are logged too
    metric_count_ignored = True         # jaccard_score over all rows (the LiDOG trainers filter label == -1 first)

    def __init__(self, model, optimizer, num_sources=1, ignore_label=-1, precision=None, sem_criterion="SoftDICELoss",
                 num_classes=7, *, sam=None, grad_clip_norm=None, sem_aux_criterion=None, sem_aux_weight=1.0):
        if num_sources not in (1, 2):
            raise NotImplementedError(f"{num_sources} sources (the reference takes one or two)")
        self.model, self.opt, self.num_sources = model, optimizer, num_sources
        self.precision = precision
        if _precision.resolve(precision):
            _precision.check_single_rank()
            self.bf16 = _precision.Bf16Training(model)
        self.sem_criterion = make_criterion(sem_criterion, ignore_label, num_classes)
        self.sem_aux_criterion = None if sem_aux_criterion is None else make_aux_criterion(sem_aux_criterion, ignore_label)
        self.sem_aux_weight = float(sem_aux_weight)
        if self.sem_aux_criterion is not None and not self.sem_aux_weight > 0:
            raise ValueError(f"sem_aux_weight = {sem_aux_weight}: the auxiliary criterion's weight is positive")
        self._prepared = {}
        if num_sources == 2:
            optimizer.buckets.set_uses(2)
        if sam is not None or grad_clip_norm is not None:
            _optim.check_single_rank("sam / grad_clip_norm")
            if sam is not None and sam.optimizer is not optimizer:
                raise ValueError("sam wraps another optimiser than the step's")
            if grad_clip_norm is not None:
                _optim.check_clip_argument(grad_clip_norm)
        self.sam, self.grad_clip_norm = sam, grad_clip_norm
        self._managers, self._replay = {}, None     # sam: the first pass's coordinate managers, by source

    def sparse_input(self, batch, s=0):
        """the SparseTensor of source `s`, on the coordinate manager prefetch_maps prepared for it if there is one"""
        key = "coords_int1" if s else "coords_int"
        coords = batch[key] if key in batch else batch[f"source_coordinates{s}"].int()
        feats = batch[f"source_features{s}"]
        if self._replay is not None:    # sam's second pass: the maps of the first, nothing is built again
            return ME.SparseTensor(features=feats, coordinates=coords, coordinate_manager=self._replay[s])
        hit = self._prepared.pop(id(coords), None)
        if hit is not None and hit[0] is coords:
            st = ME.SparseTensor(features=feats, coordinates=coords, coordinate_manager=hit[1])
        else:
            st = ME.SparseTensor(coordinates=coords, features=feats)
        if s == 0:
            self._last_manager = st.coordinate_manager
        if self.sam is not None:
            self._managers[s] = st.coordinate_manager
        return st

    def prefetch_maps(self, batch, ready=None):
        """prepare the coordinate maps of every source of `batch` (the next step's) from the trace of this step's first
        forward pass; `ready`: event after which its coordinates are valid (None: everything queued so far)"""
        if batch is None:
            return
        trace = self._last_manager.trace
        for key in ("coords_int", "coords_int1")[:self.num_sources]:
            if key in batch:
                coords = batch[key]
                self._prepared[id(coords)] = (coords, ME.CoordinateManager.prepare(coords, trace, ready))

    def point_loss(self, logits, labels):
        """the point loss of one source: the criterion, plus the weighted auxiliary criterion when there is one"""
        loss = self.sem_criterion(logits, labels)
        if self.sem_aux_criterion is not None:
            loss = loss + self.sem_aux_weight * self.sem_aux_criterion(logits, labels)
        return loss

    def _sem_losses(self, batch, outs):
        return [self.point_loss(o.F, batch[f"source_sem_labels{s}"].long()) for s, o in enumerate(outs)]

    def _named(self, **losses):
        """{"sem_loss": l} for one source, {"sem_loss0": l0, "sem_loss1": l1} for two"""
        if self.num_sources == 1:
            return {k: v[0] for k, v in losses.items()}
        return {f"{k}{s}": v[s] for k, v in losses.items() for s in (0, 1)}

    @_contextlib.contextmanager
    def _scope(self):
        """the bf16 training context of a precision="bf16" step (a stale table is packed again first); else nothing"""
        if self.bf16 is None:
            yield None
        else:
            with _precision.bf16_training(self.model, self.bf16) as ctx:
                self.precision_ctx = ctx
                yield ctx

    def _forward(self, batch, epoch):
        total, losses, outs = self._losses(batch, epoch)
        # "_TrunkFnBackward": the trunk executor took the pass
        self.last_paths = tuple(type(o.F.grad_fn).__name__ for o in outs)
        self.last_path = self.last_paths[0]
        return total, losses, outs

    def forward_loss(self, batch, epoch=0):
        """one source: (total, *losses, output); two: {"loss": total, **losses, "outputs": [output0, output1]}"""
        with self._scope():
            total, losses, outs = self._forward(batch, epoch)
        if self.num_sources == 2:
            return {"loss": total, **losses, "outputs": outs}
        return (total, *losses.values(), outs[0])

    def training_step(self, batch, epoch=0, prefetch=None, prefetch_ready=None):
        """`prefetch`: the batch of the NEXT call (its coordinate maps are built while this step still runs on
        the GPU); `prefetch_ready`: event after which its coordinates are valid (None: everything queued so far).
        Returns the detached total and losses."""
        with self._scope():
            total, losses, outs = self._forward(batch, epoch)
            ready = self.metrics.mark() if self.metrics is not None else None
            self.opt.zero_grad()
            total.backward()
            if self.sam is not None:
                self._sam_second_pass(batch, epoch)
            if self.grad_clip_norm is not None:     # the gradient the optimiser steps along: with sam, the second pass's
                self.opt.clip_grad_norm(self.grad_clip_norm)
            self.opt.step()
            if self.bf16 is not None:   # behind the step's TransposedKernels.refresh(): the dgrad table reads that copy
                self.bf16.refresh()
            if ready is not None:   # here the host is ahead of the device: most of the metrics' host time hides
                self._record_metrics(batch, total, losses, outs, ready)
            self.prefetch_maps(prefetch, prefetch_ready)     # inside the scope: work items cut for the bf16 kernel
        _check_transport(self)
        return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in {"loss": total, **losses}.items()}

    def _sam_second_pass(self, batch, epoch):
        """between the first backward pass and the optimiser step of a step with `sam`: the weights move to w + e
        (SAM.first_step), the SAME batch goes forward and backward again -- on the first pass's coordinate managers (no
        map is built twice, their traces keep the first pass's length), with the BatchNorm running statistics frozen
        (ME.frozen_running_stats) and into a new generation of the flat gradient buffer -- and the weights return
        (SAM.second_step).  Every cache of the weights follows both moves: the transposed kernels inside the SAM calls,
        the bf16 tables here.  What the step returns, logs and records stays the first pass's."""
        self.sam.first_step()
        if self.bf16 is not None:
            self.bf16.refresh()
        bev_outs = getattr(self, "_bev_outs", None)
        traces = {s: len(cm.trace) for s, cm in self._managers.items()}
        self._replay = self._managers
        try:
            with ME.frozen_running_stats():
                total, _, _ = self._forward(batch, epoch)
        finally:
            self._replay = None
            for s, cm in self._managers.items():
                del cm.trace[traces[s]:]
            self._bev_outs = bev_outs
        self.opt.zero_grad()
        total.backward()
        self.sam.second_step()
        if self.bf16 is not None:
            self.bf16.refresh()
        self._managers = {}

    def _metric_pairs(self, batch, s, out):
        """the (logits, labels) of source s that the metrics count, in the order of MetricLayout.segments"""
        return [(out.F, batch[f"source_sem_labels{s}"].long())]

    @torch.no_grad()
    def _record_metrics(self, batch, total, losses, outs, ready):
        """`ready`: the metrics' mark behind the forward pass; the logits and losses are read on the metrics' stream"""
        m = self.metrics
        pairs = [p for s, o in enumerate(outs) for p in self._metric_pairs(batch, s, o)]
        m.record(m.next_step, pairs, {"loss": total, **(losses or {"sem_loss": total})}, self.opt.lr, ready)


_PEER_CHECK_EVERY = int(_os.environ.get("LIDOG_PEER_CHECK_EVERY", "200"))


def _check_transport(step):
    """every LIDOG_PEER_CHECK_EVERY steps of a data-parallel run whose statistics take the peer all-reduce: its error
    word, agreed over the ranks (comm.Transport.check: collective, synchronises with the device) -- a rank that stopped
    sending is reported by every rank within that many steps instead of at the next epoch boundary"""
    step._n_steps = getattr(step, "_n_steps", 0) + 1
    if step._n_steps % _PEER_CHECK_EVERY or not (dist.is_available() and dist.is_initialized()):
        return
    from .comm import _TRANSPORTS
    for tr in _TRANSPORTS.values():
        if tr.peer is not None:
            tr.check()


class LiDOGStep(_Step):
    """PLTTrainer2D.training_step without the host round trips (coords / logits stay in HBM).  Per source the BEV loss
    is the mean over levels of DICE on .view(-1, C) (trainer_lighting_2d_multi.py:176-189);
    one source:  total = w0 * sem + w1 * bev,                          during warm-up total = bev;
    two sources: total = w0 * (sem0 + bev0) + w1 * (sem1 + bev1)  (:191-197), during warm-up w0 * bev0 + w1 * bev1
    (:198-205).  During warm-up the sem losses are zero tensors.
    `sem_bev_criterion`: the BEV loss by name (losses.make_bev_criterion: DICELoss, SoftDICELoss, CELoss)."""

    metric_losses = ("sem_loss", "bev_loss")
    metric_bev = True
    metric_count_ignored = False

    def __init__(self, model, optimizer, source_weights=(0.5, 0.5), warmup_epochs=0, num_classes=7, ignore_label=-1,
                 num_sources=1, precision=None, sem_criterion="SoftDICELoss", sem_bev_criterion="DICELoss", *,
                 sam=None, grad_clip_norm=None, sem_aux_criterion=None, sem_aux_weight=1.0):
        super().__init__(model, optimizer, num_sources, ignore_label, precision, sem_criterion, num_classes,
                         sem_aux_criterion=sem_aux_criterion, sem_aux_weight=sem_aux_weight, sam=sam,
                         grad_clip_norm=grad_clip_norm)
        self.w, self.warmup, self.nc = source_weights, warmup_epochs, num_classes
        self.bev_criterion = make_bev_criterion(sem_bev_criterion, ignore_label)

    def _bev_loss(self, bev, labels):
        loss = 0.0
        for key, lab in labels.items():
            # NCHW logits through .view(-1, C): reproduces trainer_lighting_2d.py:181-182 literally
            loss = loss + self.bev_criterion(bev[key].view(-1, self.nc), lab.view(-1)) / len(bev)
        return loss

    def _losses(self, batch, epoch):
        outs = [self.model(self.sparse_input(batch, s), is_train=True) for s in range(self.num_sources)]
        sems = [o[0] for o in outs]
        if self.metrics is not None:
            self._bev_outs = [o[1] for o in outs]
        bev = [self._bev_loss(o[1], batch[f"source_bev_labels{s}"]) for s, o in enumerate(outs)]
        w = self.w
        if epoch >= self.warmup:
            sem = self._sem_losses(batch, sems)
            if self.num_sources == 1:
                total = w[0] * sem[0] + w[1] * bev[0]
            else:
                total = w[0] * (sem[0] + bev[0]) + w[1] * (sem[1] + bev[1])
        else:
            sem = [torch.zeros((), device=o.F.device) for o in sems]
            total = bev[0] if self.num_sources == 1 else w[0] * bev[0] + w[1] * bev[1]
        return total, self._named(sem_loss=sem, bev_loss=bev), sems

    def _metric_pairs(self, batch, s, out):
        # a level's NCHW logits as they are: the kernel reads the flat buffer in rows of C, as .view(b, h, w, -1) does
        labels = batch[f"source_bev_labels{s}"]
        return super()._metric_pairs(batch, s, out) + [(self._bev_outs[s][lvl], labels[lvl].long())
                                                       for lvl in self.metrics.layout.levels]


class SourceStep(_Step):
    """PLTTrainer.training_step (train_source.py / Mix3D; MinkUNet34 and MinkUNet34IBN): the point loss only.
    One source: total = sem, the only loss returned; two sources (trainer_lighting.py:92-116): w0 * sem0 + w1 * sem1."""

    def __init__(self, model, optimizer, source_weights=(0.5, 0.5), ignore_label=-1, num_sources=1, precision=None,
                 sem_criterion="SoftDICELoss", num_classes=7, *, sam=None, grad_clip_norm=None, sem_aux_criterion=None,
                 sem_aux_weight=1.0):
        super().__init__(model, optimizer, num_sources, ignore_label, precision, sem_criterion, num_classes,
                         sem_aux_criterion=sem_aux_criterion, sem_aux_weight=sem_aux_weight, sam=sam,
                         grad_clip_norm=grad_clip_norm)
        self.w = source_weights

    def _losses(self, batch, epoch):
        outs = [self.model(self.sparse_input(batch, s), is_seg=True) for s in range(self.num_sources)]
        sem = self._sem_losses(batch, outs)
        if self.num_sources == 1:
            return sem[0], {}, outs
        return self.w[0] * sem[0] + self.w[1] * sem[1], self._named(sem_loss=sem), outs


class RobustStep(_Step):
    """PLTRobustNet.training_step (trainer_lighting_robustnet.py; two sources :96-150): SoftDICE on the logits, and
    from epoch `aux_epoch` (5) on the instance-whitening loss of each source's five aux maps, averaged (one launch per
    source and direction, lidog_amd.losses.iw_loss); total = w0 * sem (+ 0.5 * aux), or with two sources
    w0 * sem0 + w1 * sem1 (+ 0.5 * (aux0 + aux1)).  Before that epoch aux is a zero tensor: nothing is launched and
    nothing waits for the device."""

    metric_losses = ("sem_loss", "aux_loss")

    def __init__(self, model, optimizer, source_weights=(0.5, 0.5), aux_epoch=5, ignore_label=-1, num_sources=1,
                 precision=None, sem_criterion="SoftDICELoss", num_classes=7, *, sam=None, grad_clip_norm=None,
                 sem_aux_criterion=None, sem_aux_weight=1.0):
        super().__init__(model, optimizer, num_sources, ignore_label, precision, sem_criterion, num_classes,
                         sem_aux_criterion=sem_aux_criterion, sem_aux_weight=sem_aux_weight, sam=sam,
                         grad_clip_norm=grad_clip_norm)
        self.w, self.aux_epoch = source_weights, aux_epoch

    def _losses(self, batch, epoch):
        outs = [self.model(self.sparse_input(batch, s), is_seg=False) for s in range(self.num_sources)]
        sems = [o[0] for o in outs]
        sem = self._sem_losses(batch, sems)
        total = self.w[0] * sem[0] if self.num_sources == 1 else self.w[0] * sem[0] + self.w[1] * sem[1]
        if epoch >= self.aux_epoch:
            aux = [iw_loss([m.F for m in o[1]])[0] for o in outs]
            total = total + 0.5 * (aux[0] if self.num_sources == 1 else aux[0] + aux[1])
        else:
            aux = [torch.zeros((), device=o.F.device) for o in sems]
        return total, self._named(sem_loss=sem, aux_loss=aux), sems


def setup_data_parallel(model):
    """train_lidog.py:227-231: SyncBatchNorm conversion of the sparse BNs when world_size > 1 (the two
    BatchNorm2d of Encoder2D stay per-rank, as in the reference)."""
    if dist.is_initialized() and (dist.get_world_size() > 1 or ME.MinkowskiSyncBatchNorm.single_rank):
        model = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(model)
    return model
