"""Training step of LiDOG on the GPU: loss composition, Adam on a flat HBM buffer, RCCL data parallelism.

Restates what the reference gets from pytorch-lightning (not installable here, and python that the GPU
box never receives):
  training_step        utils/pipelines/trainer_lighting_2d.py:141-201  (PLTTrainer2D)
                       utils/pipelines/trainer_lighting.py:92-104      (PLTTrainer, source-only)
                       utils/pipelines/trainer_lighting_robustnet.py    (PLTRobustNet, one source)
  two sources          utils/pipelines/trainer_lighting_2d_multi.py:135-215 (PLTTrainer2DMulti), trainer_lighting.py:92-116,
                       trainer_lighting_robustnet.py:96-150: the *MultiStep classes below
  configure_optimizers utils/pipelines/trainer_lighting_2d.py:349-394  (Adam lr, weight_decay 1e-4)
  DDP + SyncBN         train_lidog.py:227-231,286-289                   (strategy='ddp')

One process per GPU; gradients live in ONE contiguous fp32 buffer that is all-reduced over RCCL in
a few large buckets launched as soon as their last gradient is produced (overlapping the rest of
backward), then consumed by a single fused Adam kernel.
"""
import os as _os

import torch
import torch.distributed as dist

from . import me as ME
from .losses import DICELoss, SoftDICELoss, iw_loss
from .optim import (FlatAdam, FlatParams, FlatSGD, GradientBuckets, make_optimizer, make_scheduler,  # noqa: F401
                    shard_indices)


class _CoordinatePrefetch:
    """Coordinate maps of the NEXT batch are built on a side stream while the GPU still works on the current step
    (the host runs ahead of the GPU by then): `training_step(batch, prefetch=next_batch)`.  What to build is the
    trace of map uses recorded by the first forward pass; it is the data-loader-side half of the reference's step
    (ME builds its maps inside the forward call) moved off the critical path, not skipped."""

    _trace = None

    @staticmethod
    def _coords(batch):
        return batch["coords_int"] if "coords_int" in batch else batch["source_coordinates0"].int()

    def _sparse_input(self, batch):
        coords = self._coords(batch)
        hit = self.__dict__.setdefault("_prepared", {}).pop(id(coords), None)
        if hit is not None and hit[0] is coords:
            st = ME.SparseTensor(features=batch["source_features0"], coordinates=coords, coordinate_manager=hit[1])
        else:
            st = ME.SparseTensor(coordinates=coords, features=batch["source_features0"])
        self._last_manager = st.coordinate_manager
        return st

    def _after_step(self, prefetch, prefetch_ready):
        self._trace = self._last_manager.trace
        if prefetch is not None and "coords_int" in prefetch:
            coords = prefetch["coords_int"]
            self.__dict__.setdefault("_prepared", {})[id(coords)] = \
                (coords, ME.CoordinateManager.prepare(coords, self._trace, prefetch_ready))


class _TwoSourcePrefetch(_CoordinatePrefetch):
    """_CoordinatePrefetch for batches with a second source (`source_*1`, `coords_int1`): the model is called on source 0
    and then on source 1; the trace recorded by the first call prepares the coordinate maps of BOTH inputs of the next
    batch.  The optimiser's gradient buckets expect two uses of every parameter (GradientBuckets.set_uses)."""

    def _sparse_input_of(self, batch, s):
        key = "coords_int" if s == 0 else "coords_int1"
        coords = batch[key] if key in batch else batch[f"source_coordinates{s}"].int()
        hit = self.__dict__.setdefault("_prepared", {}).pop(id(coords), None)
        feats = batch[f"source_features{s}"]
        if hit is not None and hit[0] is coords:
            st = ME.SparseTensor(features=feats, coordinates=coords, coordinate_manager=hit[1])
        else:
            st = ME.SparseTensor(coordinates=coords, features=feats)
        if s == 0:
            self._last_manager = st.coordinate_manager
        return st

    def _after_step_two(self, prefetch, prefetch_ready):
        self._trace = self._last_manager.trace
        if prefetch is None:
            return
        for key in ("coords_int", "coords_int1"):
            if key in prefetch:
                coords = prefetch[key]
                self.__dict__.setdefault("_prepared", {})[id(coords)] = \
                    (coords, ME.CoordinateManager.prepare(coords, self._trace, prefetch_ready))

    def _two_uses(self):
        buckets = getattr(self.opt, "buckets", None)
        if buckets is not None:
            buckets.set_uses(2)

    def training_step(self, batch, epoch=0, prefetch=None, prefetch_ready=None):
        """one optimiser step on both sources: the two forward passes (BatchNorm statistics move twice, source 0 first),
        ONE backward pass, one step.  Returns the detached total and per-source losses."""
        self._two_uses()
        out = self.forward_loss(batch, epoch)
        total = out["loss"]
        self.opt.zero_grad()
        total.backward()
        self.opt.step()
        self._after_step_two(prefetch, prefetch_ready)
        _check_transport(self)
        return {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items() if k not in self._not_returned}

    _not_returned = ("outputs",)


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


class LiDOGStep(_CoordinatePrefetch):
    """PLTTrainer2D.training_step without the host round trips (coords / logits stay in HBM)."""

    def __init__(self, model, optimizer, source_weights=(0.5, 0.5), warmup_epochs=0, num_classes=7, ignore_label=-1):
        self.model, self.opt = model, optimizer
        self.w, self.warmup, self.nc = source_weights, warmup_epochs, num_classes
        self.sem_criterion = SoftDICELoss(ignore_label=ignore_label)
        self.bev_criterion = DICELoss(ignore_label=ignore_label)

    def forward_loss(self, batch, epoch=0):
        st = self._sparse_input(batch)
        sem, bev = self.model(st, is_train=True)
        bev_loss = 0.0
        for key, lab in batch["source_bev_labels0"].items():
            # NCHW logits through .view(-1, C): reproduces trainer_lighting_2d.py:181-182 literally
            bev_loss = bev_loss + self.bev_criterion(bev[key].view(-1, self.nc), lab.view(-1)) / len(bev)
        if epoch >= self.warmup:
            sem_loss = self.sem_criterion(sem.F, batch["source_sem_labels0"].long())
            total = self.w[0] * sem_loss + self.w[1] * bev_loss
        else:
            sem_loss = torch.zeros((), device=sem.F.device)
            total = bev_loss
        return total, sem_loss, bev_loss, sem

    def training_step(self, batch, epoch=0, prefetch=None, prefetch_ready=None):
        """`prefetch`: the batch of the NEXT call (its coordinate maps are built while this step still runs on
        the GPU); `prefetch_ready`: event after which its coordinates are valid (None: everything queued so far)"""
        total, sem_loss, bev_loss, sem = self.forward_loss(batch, epoch)
        self.last_path = type(sem.F.grad_fn).__name__     # "_TrunkFnBackward": the trunk executor took the pass
        self.opt.zero_grad()
        total.backward()
        self.opt.step()
        self._after_step(prefetch, prefetch_ready)
        _check_transport(self)
        return {"loss": total.detach(), "sem_loss": sem_loss.detach(), "bev_loss": bev_loss.detach()}


class SourceStep(_CoordinatePrefetch):
    """PLTTrainer.training_step (train_source.py / Mix3D): MinkUNet34, SoftDICE only."""

    def __init__(self, model, optimizer, ignore_label=-1):
        self.model, self.opt = model, optimizer
        self.criterion = SoftDICELoss(ignore_label=ignore_label)

    def training_step(self, batch, epoch=0, prefetch=None, prefetch_ready=None):
        st = self._sparse_input(batch)
        out = self.model(st, is_seg=True)
        loss = self.criterion(out.F, batch["source_sem_labels0"].long())
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()
        self._after_step(prefetch, prefetch_ready)
        _check_transport(self)
        return {"loss": loss.detach()}


class RobustStep(_CoordinatePrefetch):
    """PLTRobustNet.training_step (trainer_lighting_robustnet.py) for a single source: SoftDICE on the logits, and from
    epoch `aux_epoch` (5) on the instance-whitening loss of the model's five aux maps, averaged (one launch each way,
    lidog_amd.losses.iw_loss); total = source_weights[0] * sem + 0.5 * aux.  Before that epoch aux is a zero tensor:
    nothing is launched and nothing waits for the device."""

    def __init__(self, model, optimizer, source_weights=(0.5, 0.5), aux_epoch=5, ignore_label=-1):
        self.model, self.opt = model, optimizer
        self.w, self.aux_epoch = source_weights, aux_epoch
        self.criterion = SoftDICELoss(ignore_label=ignore_label)

    def forward_loss(self, batch, epoch=0):
        st = self._sparse_input(batch)
        out, aux_maps = self.model(st, is_seg=False)
        sem_loss = self.criterion(out.F, batch["source_sem_labels0"].long())
        total = self.w[0] * sem_loss
        if epoch >= self.aux_epoch:
            aux_loss = iw_loss([m.F for m in aux_maps])[0]
            total = total + 0.5 * aux_loss
        else:
            aux_loss = torch.zeros((), device=out.F.device)
        return total, sem_loss, aux_loss, out

    def training_step(self, batch, epoch=0, prefetch=None, prefetch_ready=None):
        total, sem_loss, aux_loss, _ = self.forward_loss(batch, epoch)
        self.opt.zero_grad()
        total.backward()
        self.opt.step()
        self._after_step(prefetch, prefetch_ready)
        _check_transport(self)
        return {"loss": total.detach(), "sem_loss": sem_loss.detach(), "aux_loss": aux_loss.detach()}


def setup_data_parallel(model):
    """train_lidog.py:227-231: SyncBatchNorm conversion of the sparse BNs when world_size > 1 (the two
    BatchNorm2d of Encoder2D stay per-rank, as in the reference)."""
    if dist.is_initialized() and (dist.get_world_size() > 1 or ME.MinkowskiSyncBatchNorm.single_rank):
        model = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(model)
    return model


class LiDOGMultiStep(_TwoSourcePrefetch, LiDOGStep):
    """PLTTrainer2DMulti.training_step (trainer_lighting_2d_multi.py:135-215): the model on source 0, then on source 1;
    per source the BEV loss is the mean over levels of DICE on .view(-1, C) (:176-189);
    after warm-up  total = w0 * (sem0 + bev0) + w1 * (sem1 + bev1)   (:191-197),
    during warm-up total = w0 * bev0 + w1 * bev1                     (:198-205)."""

    def forward_loss(self, batch, epoch=0):
        outs = [self.model(self._sparse_input_of(batch, s), is_train=True) for s in (0, 1)]
        bev_l, sem_l = [], []
        for s, (sem, bev) in enumerate(outs):
            loss = 0.0
            for key, lab in batch[f"source_bev_labels{s}"].items():
                loss = loss + self.bev_criterion(bev[key].view(-1, self.nc), lab.view(-1)) / len(bev)
            bev_l.append(loss)
        if epoch >= self.warmup:
            sem_l = [self.sem_criterion(outs[s][0].F, batch[f"source_sem_labels{s}"].long()) for s in (0, 1)]
            total = self.w[0] * (sem_l[0] + bev_l[0]) + self.w[1] * (sem_l[1] + bev_l[1])
        else:
            sem_l = [torch.zeros((), device=outs[s][0].F.device) for s in (0, 1)]
            total = self.w[0] * bev_l[0] + self.w[1] * bev_l[1]
        self.last_paths = tuple(type(o[0].F.grad_fn).__name__ for o in outs)
        self.last_path = self.last_paths[0]
        return {"loss": total, "sem_loss0": sem_l[0], "bev_loss0": bev_l[0], "sem_loss1": sem_l[1],
                "bev_loss1": bev_l[1], "outputs": [o[0] for o in outs]}


class SourceMultiStep(_TwoSourcePrefetch, SourceStep):
    """PLTTrainer.training_step with two sources (trainer_lighting.py:92-116; MinkUNet34 and MinkUNet34IBN):
    total = w0 * sem0 + w1 * sem1."""

    def __init__(self, model, optimizer, source_weights=(0.5, 0.5), ignore_label=-1):
        super().__init__(model, optimizer, ignore_label=ignore_label)
        self.w = source_weights

    def forward_loss(self, batch, epoch=0):
        outs = [self.model(self._sparse_input_of(batch, s), is_seg=True) for s in (0, 1)]
        sem_l = [self.criterion(outs[s].F, batch[f"source_sem_labels{s}"].long()) for s in (0, 1)]
        total = self.w[0] * sem_l[0] + self.w[1] * sem_l[1]
        self.last_paths = tuple(type(o.F.grad_fn).__name__ for o in outs)
        return {"loss": total, "sem_loss0": sem_l[0], "sem_loss1": sem_l[1], "outputs": outs}


class RobustMultiStep(_TwoSourcePrefetch, RobustStep):
    """PLTRobustNet.training_step with two sources (trainer_lighting_robustnet.py:96-150):
    total = w0 * sem0 + w1 * sem1 + 0.5 * (aux0 + aux1), aux_s the mean IWLoss of source s's five aux maps from epoch
    `aux_epoch` (5) on -- one iw_loss launch per source and direction (at most 8 maps per launch) -- else zero."""

    def forward_loss(self, batch, epoch=0):
        outs = [self.model(self._sparse_input_of(batch, s), is_seg=False) for s in (0, 1)]
        sem_l = [self.criterion(outs[s][0].F, batch[f"source_sem_labels{s}"].long()) for s in (0, 1)]
        total = self.w[0] * sem_l[0] + self.w[1] * sem_l[1]
        if epoch >= self.aux_epoch:
            aux_l = [iw_loss([m.F for m in outs[s][1]])[0] for s in (0, 1)]
            total = total + 0.5 * (aux_l[0] + aux_l[1])
        else:
            aux_l = [torch.zeros((), device=outs[s][0].F.device) for s in (0, 1)]
        self.last_paths = tuple(type(o[0].F.grad_fn).__name__ for o in outs)
        return {"loss": total, "sem_loss0": sem_l[0], "sem_loss1": sem_l[1], "aux_loss0": aux_l[0],
                "aux_loss1": aux_l[1], "outputs": [o[0] for o in outs]}
