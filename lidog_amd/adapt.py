"""Test-time adaptation: the model adapts to an unlabelled target while it is being evaluated.  Not in the reference.

  bn      prediction-time BatchNorm (Nado et al. 2020): every test batch is normalised with its own statistics
  adabn   AdaBN (Li et al. 2016): the BatchNorm running statistics are re-estimated on the target scans first
          (TestTimeAdapter.estimate), then the evaluation is the usual one
  tent    TENT (Wang et al., ICLR 2021): `bn`, and one gradient step per test batch on the norm layers' affine parameters
          that lowers the entropy of the batch's predictions (losses.EntropyLoss, csrc/entropy.hip)

A TestTimeAdapter is called like evaluate.Predictor and takes its place in evaluate.TargetEvaluator(adapter=...).  The
adapting forward pass is the training-mode forward on the operator path with is_train false (no BEV head) under
me.frozen_running_stats(): a model with frozen parameters never reaches the trunk executor.  One rank, fp32.
No gain in mIoU is promised or measured; the tests hold the arithmetic, not the benefit.
"""
import torch

from . import me as ME
from . import optim as _optim
from . import precision as _precision
from .evaluate import Predictor
from .losses import EntropyLoss

MODES = ("bn", "adabn", "tent")


def norm_parameters(model):
    """the weight and bias of every MinkowskiBatchNorm / MinkowskiSyncBatchNorm / MinkowskiInstanceNorm of `model`, in
    model.parameters() order: what TENT updates.  The BatchNorm2d layers of MinkUNet34BEV's 2-D head are not among them:
    the evaluation forward (is_train false) does not pass through that head."""
    ids = set()
    for m in model.modules():
        holder = m.bn if isinstance(m, ME.MinkowskiBatchNorm) else m if isinstance(m, ME.MinkowskiInstanceNorm) else None
        if holder is not None:
            ids.update(id(p) for p in (holder.weight, holder.bias) if p is not None)
    return [p for p in model.parameters() if id(p) in ids]


def batch_norms(model):
    """the torch BatchNorm module inside every MinkowskiBatchNorm of `model`, in model.modules() order"""
    return [m.bn for m in model.modules() if isinstance(m, ME.MinkowskiBatchNorm)]


def _batch_of(item):
    return item[0] if isinstance(item, (tuple, list)) else item


class TestTimeAdapter:
    """adapter(coords, feats, next_coords=None) -> (preds, logits), `.output` the output SparseTensor: evaluate.Predictor's
    calling convention, the next batch's coordinate maps built on the side stream included.

    bn: a training-mode forward under me.frozen_running_stats() and torch.no_grad(); no byte of the model changes.
    tent: at construction every parameter outside norm_parameters(model) gets requires_grad_(False) (and keeps it) and
      optim.make_optimizer(`optimizer`, lr, weight decay 0) is built over the rest; per batch, `steps` times: the bn
      forward with autograd on, EntropyLoss(margin), backward, optimiser step.  The logits returned are the first
      forward's, from before any update of that batch (TENT's rule); the running statistics stay frozen.
    adabn: estimate(batches) first; calls are plain evaluation forwards after it.
    reset() puts the model and the optimiser back to their bytes at construction (eval_target: once per target).
    `margin`: EntropyLoss's, an absolute entropy (None: every row takes part)."""

    __test__ = False      # not a test class, whatever its name starts with

    def __init__(self, model, mode, lr=1e-3, optimizer="Adam", steps=1, margin=None):
        if mode not in MODES:
            raise ValueError(f"TestTimeAdapter: mode={mode!r} (one of {', '.join(MODES)})")
        if int(steps) < 1:
            raise ValueError(f"TestTimeAdapter: steps={steps} (at least 1)")
        _optim.check_single_rank("TestTimeAdapter")
        self.model, self.mode, self.steps = model, mode, int(steps)
        self.output = None
        self.kernels = None           # Predictor's bf16 table: adaptation is fp32 only
        self.bns = batch_norms(model)
        self.opt = self.criterion = None
        self._next = self._trace = self._plain = None
        self._estimated = False
        if mode == "tent":
            keep = {id(p) for p in norm_parameters(model)}
            if not keep:
                raise ValueError("TestTimeAdapter: the model has no norm layer with affine parameters to adapt")
            for p in model.parameters():
                if id(p) not in keep:
                    p.requires_grad_(False)
            self.opt = _optim.make_optimizer(optimizer, model, lr, weight_decay=0.0)
            self.criterion = EntropyLoss(margin)
        elif mode == "adabn":
            self._plain = Predictor(model)
        self._snapshot()

    # ------------------------------------------------------------------ the state at construction
    def _snapshot(self):
        self._state = {k: v.detach().clone() for k, v in self.model.state_dict().items()}
        if self.opt is not None:
            self._opt_state = {k: getattr(self.opt, k).clone() for k in self.opt._state}
            self._opt_host = (self.opt.lr, self.opt.base_lr, list(self.opt.param_steps))

    @torch.no_grad()
    def reset(self):
        """every byte of the parameters, the buffers and the optimiser state as at construction; the transposed kernels
        the backward pass caches are refreshed.  An adabn adapter needs estimate() again."""
        for k, v in self.model.state_dict().items():      # taking it flushes the host-side batch counters first
            v.copy_(self._state[k])
        if self.opt is not None:
            for k, v in self._opt_state.items():
                getattr(self.opt, k).copy_(v)
            self.opt.lr, self.opt.base_lr, steps = self._opt_host
            self.opt.param_steps = list(steps)
            self.opt.zero_grad()
            self.opt.transposed.refresh()
        self._estimated = False

    # ------------------------------------------------------------------ the adapting forward pass
    def _forward(self, coords, feats, manager, frozen=True):
        """the model's output SparseTensor of a training-mode forward (is_train false): batch statistics in every
        BatchNorm; `frozen`: the running statistics stay what they are"""
        if _precision.current() is not None:
            raise ValueError("TestTimeAdapter: a bf16 table is current; test-time adaptation is fp32 only")
        model = self.model
        if manager is None and self._trace is not None:
            manager = ME.CoordinateManager.prepare(coords, self._trace)
        if manager is not None:
            st = ME.SparseTensor(features=feats, coordinates=coords, coordinate_manager=manager)
        else:
            st = ME.SparseTensor(coordinates=coords, features=feats)
        was_training = model.training
        model.train()
        try:
            if frozen:
                with ME.frozen_running_stats():
                    out = model(st)
            else:
                out = model(st)
        finally:
            model.train(was_training)
        if self._trace is None:
            self._trace = list(st.coordinate_manager.trace)
        return out[0] if isinstance(out, tuple) else out

    def __call__(self, coords, feats, next_coords=None):
        if self.mode == "adabn":
            if not self._estimated:
                raise RuntimeError("TestTimeAdapter('adabn'): call estimate(batches) before the scored pass")
            out = self._plain(coords, feats, next_coords)
            self.output = self._plain.output
            return out
        mgr = None
        if self._next is not None and self._next[0] is coords:
            mgr = self._next[1]
        self._next = None
        ready = torch.cuda.Event()       # the next batch's coordinates are valid now (Predictor.__call__)
        ready.record()
        if self.mode == "bn":
            with torch.no_grad():
                first = self._forward(coords, feats, mgr)
        else:
            first = self._tent(coords, feats, mgr)
        self.output = first
        if next_coords is not None and self._trace is not None:
            self._next = (next_coords, ME.CoordinateManager.prepare(next_coords, self._trace, ready))
        return first.F.max(dim=1)[1], first.F

    def _tent(self, coords, feats, mgr):
        if coords.shape[0] < 2:
            raise ValueError(f"TestTimeAdapter('tent'): a batch of {coords.shape[0]} rows (batch statistics need 2)")
        first = None
        with torch.enable_grad():
            for _ in range(self.steps):
                self.opt.zero_grad()
                out = self._forward(coords, feats, mgr)
                mgr = out.coordinate_manager          # the maps of a batch are built once
                if first is None:
                    first = out._like(out.F.detach())
                self.criterion(out.F).backward()
                self.opt.step()
        return first

    # ------------------------------------------------------------------ AdaBN
    @torch.no_grad()
    def estimate(self, batches):
        """AdaBN: every BatchNorm's running statistics reset to (0, 1), then batch k = 0, 1, ... of `batches` (batch
        dicts, or the (batch, scan indices) pairs of evaluate.dataset_batches) through a training-mode forward with every
        momentum set to 1 / (k + 1) on the host: the running statistics end as the mean of the batches' means and
        unbiased variances -- torch's momentum=None rule without a read of num_batches_tracked from the device.  The
        modules' own momenta return afterwards.  Returns the number of batches."""
        if self.mode != "adabn":
            raise RuntimeError(f"TestTimeAdapter({self.mode!r}).estimate: only the adabn mode estimates")
        saved = [bn.momentum for bn in self.bns]
        for bn in self.bns:
            if bn.track_running_stats and bn.running_mean is not None:
                bn._nbt_pending = 0
                bn.running_mean.zero_()
                bn.running_var.fill_(1.0)
                bn.num_batches_tracked.zero_()
        k = 0
        try:
            for item in batches:
                b = _batch_of(item)
                for bn in self.bns:
                    bn.momentum = 1.0 / (k + 1)
                self._forward(b["coords_int"], b["source_features0"], None, frozen=False)
                k += 1
        finally:
            for bn, momentum in zip(self.bns, saved):
                bn.momentum = momentum
        if k == 0:
            raise ValueError("TestTimeAdapter.estimate: no batches")
        self._estimated = True
        return k
