"""The training criteria, kept on the device (the reference moves logits to the CPU first).

  SoftDICELoss  utils/losses/losses.py:100-126,129-187  (powerize, present-class mask, eps = 0.05; is_kitti: the
                                                         19-class soft labels that pair classes 1 and 6)
  DICELoss      utils/losses/losses.py:56-97            (hard one-hot, no mask)
  CELoss        utils/losses/losses.py:8-25             (nn.CrossEntropyLoss(weight, ignore_index), mean)
  FocalLoss     utils/losses/losses.py:423-436          (alpha (1 - exp(-ce))^gamma ce on that mean)
  make_criterion / make_bev_criterion                   (init_losses of utils/pipelines/trainer_lighting*.py)
  LovaszSoftmaxLoss / make_aux_criterion                (not in the reference: Berman et al., CVPR 2018, added to the
                                                         point criterion of a step; csrc/lovasz.hip)
  IWLoss        utils/losses/losses.py:464-485          (RobustNet's instance-whitening loss, csrc/iwloss.hip)
  CovMatrix_IRW utils/models/cov_settings.py:4-25        (its eye / mask helper)
Same formulas as the reference, as HIP kernels (csrc/losses.hip; there is no torch formula behind them: CPU tensors and
unsupported class counts raise); the `.cpu()` round trips (losses.py:72-73,148-149) are gone, and rows carrying the
ignore label are skipped in place instead of being compacted away with boolean indexing: the compaction needs the
number of valid rows on the host, i.e. a device synchronisation in the middle of every step.
"""
import ctypes

import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr

_FUSED_CLASSES = tuple(range(2, 21))   # csrc/losses.hip: one instantiation per class count (the reference uses 7)


class _DiceFn(torch.autograd.Function):
    """csrc/losses.hip: softmax + the per-class sums in one pass, the gradient in one pass"""

    @staticmethod
    def forward(ctx, logits, target, ignore_label, eps, soft, powerize, use_tmask, offset, kitti=False):
        logits, target = logits.contiguous(), target.contiguous()
        if target.dtype != torch.int64:
            target = target.long()
        n, C = logits.shape
        dev = logits.device
        ws = torch.empty(_lib.load().lidog_dice_ws(C), dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(2 * C, dtype=torch.float32, device=dev)
        has_ignore = ignore_label is not None
        cfg = (n, C, int(ignore_label) if has_ignore else 0, 1 if has_ignore else 0, float(eps))
        cfg += (1 if powerize else 0,) if kitti else (1 if soft else 0, 1 if powerize else 0)   # the KITTI entry is soft
        call("lidog_dice_kitti_fwd" if kitti else "lidog_dice_fwd", ptr(logits), ptr(target), *cfg,
             1 if use_tmask else 0, float(offset), ptr(ws), ptr(loss), ptr(coef))
        ctx.save_for_backward(logits, target, coef)
        ctx.cfg, ctx.kitti = cfg, kitti
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, target, coef = ctx.saved_tensors
        g = torch.empty_like(logits)
        call("lidog_dice_kitti_bwd" if ctx.kitti else "lidog_dice_bwd", ptr(logits), ptr(target), *ctx.cfg, ptr(coef),
             ptr(gout.contiguous()), ptr(g))
        return g, None, None, None, None, None, None, None, None


def _check(output):
    """the criteria exist as HIP kernels only (csrc/losses.hip): no torch formula behind them"""
    _lib.require_gpu(output, "logits")
    if output.dim() != 2 or output.shape[1] not in _FUSED_CLASSES or output.dtype != torch.float32:
        raise NotImplementedError(f"lidog_amd DICE losses take float32 logits [n, C] with C in {_FUSED_CLASSES}, "
                                  f"got {tuple(output.shape)} {output.dtype}")


class SoftDICELoss(nn.Module):
    def __init__(self, ignore_label=None, powerize=True, use_tmask=True, neg_range=False, eps=0.05, is_kitti=False):
        super().__init__()
        self.ignore_label, self.powerize, self.use_tmask, self.neg_range, self.eps, self.is_kitti = \
            ignore_label, powerize, use_tmask, neg_range, eps, is_kitti

    def forward(self, output, target, is_kitti=False):
        """`is_kitti` here or in the constructor: get_kitti_soft's targets (a row labelled 1 or 6 carries (1 - eps) / 2
        on classes 1 and 6 both), which need C >= 7"""
        _check(output)
        kitti = bool(self.is_kitti or is_kitti)
        if kitti and output.shape[1] < 7:
            raise ValueError(f"SoftDICELoss(is_kitti=True) pairs classes 1 and 6: C = {output.shape[1]} < 7")
        return _DiceFn.apply(output, target, self.ignore_label, self.eps, True, self.powerize, self.use_tmask,
                             -1.0 if self.neg_range else 0.0, kitti)


class DICELoss(nn.Module):
    def __init__(self, ignore_label=None, powerize=False, use_tmask=False):
        super().__init__()
        self.ignore_label, self.powerize, self.use_tmask = ignore_label, powerize, use_tmask

    def forward(self, output, target):
        _check(output)
        return _DiceFn.apply(output, target, self.ignore_label, 0.0, False, self.powerize, self.use_tmask, 0.0)


# ------------------------------------------------------------------ cross-entropy and focal loss
class _CEFn(torch.autograd.Function):
    """csrc/losses.hip: the weighted log-sum-exp sums in one pass, the gradient in one pass; `focal`: None or
    (alpha, gamma)"""

    @staticmethod
    def forward(ctx, logits, target, ignore_label, weight, focal):
        logits, target = logits.contiguous(), target.contiguous()
        if target.dtype != torch.int64:
            target = target.long()
        n, C = logits.shape
        dev = logits.device
        ws = torch.empty(_lib.load().lidog_ce_ws(C), dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(1, dtype=torch.float32, device=dev)
        has_ignore = ignore_label is not None
        cfg = (n, C, int(ignore_label) if has_ignore else 0, 1 if has_ignore else 0, ptr(weight))
        alpha, gamma = focal if focal is not None else (1.0, 0.0)
        call("lidog_ce_fwd", ptr(logits), ptr(target), *cfg, 0 if focal is None else 1, float(alpha), float(gamma),
             ptr(ws), ptr(loss), ptr(coef))
        ctx.save_for_backward(logits, target, coef)
        ctx.cfg, ctx.weight = cfg, weight       # the table itself: cfg holds its address only
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, target, coef = ctx.saved_tensors
        g = torch.empty_like(logits)
        call("lidog_ce_bwd", ptr(logits), ptr(target), *ctx.cfg, ptr(coef), ptr(gout.contiguous()), ptr(g))
        return g, None, None, None, None


class _WeightedCE(nn.Module):
    """what CELoss and FocalLoss share: the class-weight table, uploaded once, and the checks"""

    def __init__(self, ignore_label, weight):
        super().__init__()
        self.ignore_label = ignore_label
        if weight is not None:
            weight = torch.as_tensor(weight).detach().float().contiguous()
            if weight.dim() != 1:
                raise ValueError(f"the class weights are a vector [C], got {tuple(weight.shape)}")
            if not weight.is_cuda:
                weight = weight.cuda() if torch.cuda.is_available() else weight
        self.register_buffer("weight", weight, persistent=False)

    def _apply_fn(self, output, target, focal):
        _check(output)
        w = self.weight
        if w is not None:
            if w.shape[0] != output.shape[1]:
                raise ValueError(f"{w.shape[0]} class weights for logits with C = {output.shape[1]}")
            if w.device != output.device:       # a module built before the GPU was there, or moved
                self.weight = w = w.to(output.device)
        return _CEFn.apply(output, target, self.ignore_label, w, focal)


class CELoss(_WeightedCE):
    """nn.CrossEntropyLoss(weight, ignore_index=ignore_label), mean reduction.  `weight`: numpy array (as in the
    reference) or tensor [C]; `ignore_label=None`: no row is ignored.  A label outside [0, C) other than the ignore label
    takes no part (torch asserts on the device)."""

    def __init__(self, ignore_label=None, weight=None):
        super().__init__(ignore_label, weight)

    def forward(self, preds, gt):
        return self._apply_fn(preds, gt, None)


class FocalLoss(_WeightedCE):
    """-(1 - pt)^gamma alpha log pt with log pt = -CE(preds, labels), the mean cross-entropy: a scalar function of it"""

    def __init__(self, alpha=0.5, gamma=2, weight=None, ignore_index=-1):
        super().__init__(ignore_index, weight)
        self.alpha, self.gamma, self.ignore_index = alpha, gamma, ignore_index

    def forward(self, preds, labels):
        return self._apply_fn(preds, labels, (self.alpha, self.gamma))


POINT_CRITERIA = ("CELoss", "DICELoss", "SoftDICELoss", "FocalLoss")
BEV_CRITERIA = ("DICELoss", "SoftDICELoss", "CELoss")


def make_criterion(name, ignore_label=-1, num_classes=7):
    """losses.sem_criterion of init_losses (trainer_lighting.py:73-90): FocalLoss is (alpha 0.25, gamma 2) and keeps its
    own default ignore_index of -1, as there; SoftDICELoss takes the KITTI soft labels as soon as num_classes == 19; any
    other name raises"""
    if name == "CELoss":
        return CELoss(ignore_label=ignore_label, weight=None)
    if name == "DICELoss":
        return DICELoss(ignore_label=ignore_label)
    if name == "SoftDICELoss":
        return SoftDICELoss(ignore_label=ignore_label, is_kitti=num_classes == 19)
    if name == "FocalLoss":
        return FocalLoss(alpha=0.25, gamma=2)
    raise NotImplementedError(f"sem_criterion {name!r}: one of {POINT_CRITERIA}")


def make_bev_criterion(name, ignore_label=-1):
    """losses.sem_bev_criterion of init_losses (trainer_lighting_2d.py:107-116; SoftDICELoss without the KITTI rule, as
    there).  The reference falls through to CELoss for every other name; here another name raises."""
    if name == "DICELoss":
        return DICELoss(ignore_label=ignore_label)
    if name == "SoftDICELoss":
        return SoftDICELoss(ignore_label=ignore_label)
    if name == "CELoss":
        return CELoss(ignore_label=ignore_label, weight=None)
    raise NotImplementedError(f"sem_bev_criterion {name!r}: one of {BEV_CRITERIA}")


# ------------------------------------------------------------------ Lovasz-softmax, the auxiliary point criterion
class _LovaszFn(torch.autograd.Function):
    """csrc/lovasz.hip: errors, one radix sort of the C n (error, row) pairs, an integer prefix count and the Jaccard
    gradient g forward; one pass per row backward.  The launches depend on the shape alone: nothing is read back."""

    @staticmethod
    def forward(ctx, logits, target, ignore_label):
        logits, target = logits.contiguous(), target.contiguous()
        if target.dtype != torch.int64:
            target = target.long()
        n, C = logits.shape
        dev = logits.device
        ws = torch.empty(_lib.load().lidog_lovasz_ws(n, C), dtype=torch.uint8, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(n * C + 1, dtype=torch.float32, device=dev)      # the tail word: 1 / present classes
        has_ignore = ignore_label is not None
        cfg = (n, C, int(ignore_label) if has_ignore else 0, 1 if has_ignore else 0)
        call("lidog_lovasz_fwd", ptr(logits), ptr(target), *cfg, ptr(ws), ptr(loss), ptr(coef), None)
        ctx.save_for_backward(logits, target, coef)
        ctx.cfg = cfg
        return loss

    @staticmethod
    def backward(ctx, gout):
        logits, target, coef = ctx.saved_tensors
        g = torch.empty_like(logits)
        call("lidog_lovasz_bwd", ptr(logits), ptr(target), *ctx.cfg, ptr(coef), ptr(coef[logits.numel():]),
             ptr(gout.contiguous()), ptr(g))
        return g, None, None


class LovaszSoftmaxLoss(nn.Module):
    """Lovasz-softmax (Berman et al., CVPR 2018), lovasz_softmax_flat with classes='present': the mean over the classes
    that a valid row carries of the Lovasz extension of the Jaccard loss on the errors |[t == c] - softmax(x)_c|.  A row
    is valid when its label is not `ignore_label` (None: no row is ignored) and lies in [0, C), CELoss's rule.  The
    surrogate of the mIoU; used next to a point criterion (make_aux_criterion), not in place of one."""

    def __init__(self, ignore_label=None):
        super().__init__()
        self.ignore_label = ignore_label

    def forward(self, output, target):
        _check(output)
        return _LovaszFn.apply(output, target, self.ignore_label)


AUX_CRITERIA = ("LovaszSoftmaxLoss",)


def make_aux_criterion(name, ignore_label=-1):
    """the auxiliary point criterion of a training step by name (trainer._Step: sem_aux_criterion): it is ADDED to the
    step's point criterion, times a weight.  Not in the reference; any other name raises."""
    if name == "LovaszSoftmaxLoss":
        return LovaszSoftmaxLoss(ignore_label=ignore_label)
    raise NotImplementedError(f"sem_aux_criterion {name!r}: one of {AUX_CRITERIA}")


# ------------------------------------------------------------------ entropy, the criterion of test-time adaptation
class _EntropyFn(torch.autograd.Function):
    """csrc/entropy.hip: every row's entropy and the sum over the rows that take part in one pass, the gradient in one
    pass.  Returns (loss, row_h, taken); only the loss carries a gradient."""

    @staticmethod
    def forward(ctx, logits, mask, margin):
        logits = logits.contiguous()
        n, C = logits.shape
        dev = logits.device
        ws = torch.empty(_lib.load().lidog_entropy_ws(C), dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        coef = torch.empty(2, dtype=torch.float32, device=dev)
        row_h = torch.empty(n, dtype=torch.float32, device=dev)
        call("lidog_entropy_fwd", ptr(logits), ptr(mask), n, C, margin, ptr(ws), ptr(loss), ptr(coef), ptr(row_h))
        ctx.save_for_backward(logits, coef, row_h)
        ctx.mask, ctx.margin = mask, margin
        taken = coef[1]
        ctx.mark_non_differentiable(row_h, taken)
        return loss, row_h, taken

    @staticmethod
    def backward(ctx, gout, _row_h, _taken):
        logits, coef, row_h = ctx.saved_tensors
        n, C = logits.shape
        g = torch.empty_like(logits)
        call("lidog_entropy_bwd", ptr(logits), ptr(ctx.mask), ptr(row_h), n, C, ctx.margin, ptr(coef),
             ptr(gout.contiguous()), ptr(g))
        return g, None, None


class EntropyLoss(nn.Module):
    """The mean Shannon entropy of softmax(logits) over the rows that take part: what TENT (Wang et al., ICLR 2021)
    minimises on unlabelled batches (lidog_amd.adapt.TestTimeAdapter); it takes no labels and is no --sem-criterion.
    `mask` ([n] bool or uint8, None: every row) and `margin` (None or <= 0: off; else only rows whose entropy lies below
    it take part, the reliable-sample filter of EATA / SAR, usually 0.4 ln C) choose the rows; with none the loss is 0.
    After a call `row_entropy` holds every row's entropy ([n] float32, rows that take no part included) and `taken` the
    number of rows that took part (a 0-dim float tensor on the device: nothing is read back)."""

    def __init__(self, margin=None):
        super().__init__()
        self.margin = 0.0 if margin is None else float(margin)
        self.row_entropy = self.taken = None

    def forward(self, logits, mask=None):
        _check(logits)
        if mask is not None:
            _lib.require_gpu(mask, "mask")
            if mask.shape != (logits.shape[0],) or mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError(f"EntropyLoss: mask must be bool or uint8 [{logits.shape[0]}], got {mask.dtype} "
                                 f"{tuple(mask.shape)}")
            mask = mask.contiguous().view(torch.uint8)
        loss, self.row_entropy, self.taken = _EntropyFn.apply(logits, mask, self.margin)
        return loss


# ------------------------------------------------------------------ instance-whitening loss (RobustNet)
# IWLoss views a map [n, C] as [n, C, 1]: its "covariance" is one C x C outer product per ROW, over all rows of all scans
# together, masked to the strict upper triangle, |.|-summed and divided by n (n - 1) (csrc/iwloss.hip has the closed
# form).  n < 2 divides by zero in the reference; here it raises ValueError before any launch.  `margin` and
# `num_remove_cov` of CovMatrix_IRW are unused, as in the reference.
IW_MAX_MAPS = 8


def _iw_args(maps):
    M = len(maps)
    xs = (ctypes.c_void_p * M)(*[m.data_ptr() for m in maps])
    ns = (ctypes.c_int64 * M)(*[m.shape[0] for m in maps])
    cs = (ctypes.c_int32 * M)(*[m.shape[1] for m in maps])
    ws = (ctypes.c_double * M)(*[1.0 / (m.shape[0] * (m.shape[0] - 1.0)) for m in maps])
    return xs, ns, cs, ws, M


class _IWFn(torch.autograd.Function):
    """csrc/iwloss.hip: every map in one launch each way; total = scale * sum_m L(map m), per-map L undifferentiated"""

    @staticmethod
    def forward(ctx, scale, *maps):
        dev = maps[0].device
        xs, ns, cs, ws, M = _iw_args(maps)
        total = torch.empty((), dtype=torch.float32, device=dev)
        per_map = torch.empty(M, dtype=torch.float32, device=dev)
        wsp = torch.empty(_lib.load().lidog_iw_ws(), dtype=torch.float64, device=dev)
        call("lidog_iw_fwd", xs, ns, cs, ws, M, float(scale), ptr(wsp), ptr(total), ptr(per_map))
        ctx.save_for_backward(*maps)
        ctx.scale = scale
        ctx.mark_non_differentiable(per_map)
        return total, per_map

    @staticmethod
    def backward(ctx, gout, _unused):
        maps = ctx.saved_tensors
        xs, ns, cs, ws, M = _iw_args(maps)
        grads = [torch.empty_like(m) for m in maps]
        gx = (ctypes.c_void_p * M)(*[g.data_ptr() for g in grads])
        call("lidog_iw_bwd", xs, ns, cs, ws, M, float(ctx.scale), ptr(gout.contiguous()), gx)
        return (None, *grads)


def _iw_check(f_map):
    _lib.require_gpu(f_map, "IWLoss feature map")
    if f_map.dim() != 2 or f_map.dtype != torch.float32:
        raise NotImplementedError(f"IWLoss takes float32 feature maps [n, C], got {tuple(f_map.shape)} {f_map.dtype}")
    if f_map.shape[0] < 2:
        raise ValueError(f"IWLoss needs n >= 2 rows (the reference divides by n - 1), got n = {f_map.shape[0]}")
    if f_map.shape[1] < 1:
        raise ValueError("IWLoss needs C >= 1 channels")
    return f_map.contiguous()


def iw_loss(maps, scale=None):
    """(scale * sum_m IWLoss(maps[m]), per-map IWLoss values [M]) with one launch each way; scale defaults to 1 / M
    (the mean of PLTRobustNet.training_step's aux loss).  Only the first output carries a gradient."""
    maps = [_iw_check(m) for m in maps]
    if not 1 <= len(maps) <= IW_MAX_MAPS:
        raise ValueError(f"iw_loss takes 1 to {IW_MAX_MAPS} maps per launch, got {len(maps)}")
    scale = 1.0 / len(maps) if scale is None else float(scale)
    return _IWFn.apply(scale, *maps)


class IWLoss(nn.Module):
    """IWLoss (utils/losses/losses.py:464-485), reference call signature.  eye / mask_matrix must be what CovMatrix_IRW
    gives (the identity -- or None -- and ones(C, C).triu(1)): any other mask raises.  margin and num_remove_cov are
    unused, as in the reference."""

    def forward(self, f_map, eye, mask_matrix, margin=None, num_remove_cov=None):
        f = _iw_check(f_map)
        C = f.shape[1]
        want = torch.ones((C, C), dtype=mask_matrix.dtype, device=mask_matrix.device).triu(1)
        if tuple(mask_matrix.shape) != (C, C) or not torch.equal(mask_matrix, want):
            raise ValueError("IWLoss: the closed form needs mask_matrix = ones(C, C).triu(1) (CovMatrix_IRW's mask)")
        return iw_loss([f], scale=1.0)[0]


class CovMatrix_IRW:
    """utils/models/cov_settings.py: (eye, strict upper-triangle mask, margin, number of off-diagonal entries) of a
    feature map's channel count, on the map's device"""

    def __init__(self, relax_denom=2.0):
        self.relax_denom = relax_denom

    def __call__(self, feats):
        dim = feats.shape[1]
        self.dim = dim
        self.i = torch.eye(dim, dim, device=feats.device)
        self.reversal_i = torch.ones((dim, dim), device=feats.device).triu(diagonal=1)
        self.num_off_diagonal = torch.sum(self.reversal_i)
        self.margin = 0 if self.relax_denom == 0 else self.num_off_diagonal // self.relax_denom
        return self.i, self.reversal_i, self.margin, self.num_off_diagonal
