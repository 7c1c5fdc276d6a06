"""Opt-in bf16 inference: the evaluation passes' sparse convolutions on the bf16 matrix instruction.

The reference passes `pipeline.precision` to Lightning's Trainer; here the knob covers evaluation only.  Activations stay
fp32 in memory (every BatchNorm, residual, ReLU, concatenation, instance-norm and metric kernel is untouched); a
convolution whose channel counts are multiples of 32 multiplies bf16 operands with fp32 accumulation
(csrc/sconv_bf16.hip): the gathered rows are rounded as they are staged, the weights are packed once per run.

    with bf16_inference(model) as ctx:            # packs; or bf16_inference(model, kernels) with a Bf16Kernels
        preds, logits = evaluate.predict(model, coords, feats)
    ctx.launches                                  # Counter: route -> convolutions that took it

A packed table is a SNAPSHOT of the weights.  Its validity is not tied to the parameters' version counters: the
optimiser's HIP kernels write through raw pointers and never advance them.  Whoever owns a Bf16Kernels calls refresh()
after the weights change.  Without a current table (the default) no code path changes."""
import collections
import contextlib
import threading

import torch

from ._lib import call, ptr, require_gpu

PRECISIONS = (None, "fp32", "bf16")
_state = threading.local()


def resolve(precision):
    """True for "bf16", False for "fp32", None for None; anything else is a ValueError"""
    if precision not in PRECISIONS:
        raise ValueError(f"precision={precision!r} (one of None, 'fp32', 'bf16')")
    return None if precision is None else precision == "bf16"


def eligible(conv):
    """THE rule: a sparse convolution takes the bf16 route when both channel counts are multiples of 32 (two MFMAs of
    16 channels per 32-channel chunk, 32-column tiles).  For MinkUNet34 and its variants that is every convolution but
    the 5^3 stem (Cin = 1) and the classifier (96 -> 7)."""
    from . import me
    return isinstance(conv, me._ConvBase) and conv.in_channels > 0 and conv.out_channels > 0 and \
        conv.in_channels % 32 == 0 and conv.out_channels % 32 == 0


class Bf16Kernels:
    """bf16 [K, Cout, Cin] copies of the kernels [K, Cin, Cout] of every eligible convolution of `model` (transposed:
    a lane's eight k-values of the B operand are 16 contiguous bytes), written by ONE launch of lidog_pack_kernels_bf16
    on construction and on every refresh()."""

    def __init__(self, model):
        self.convs = [m for m in model.modules() if eligible(m)]
        if not self.convs:
            raise ValueError("Bf16Kernels: the model has no convolution with channel counts that are multiples of 32")
        for c in self.convs:
            require_gpu(c.kernel, "the model of a bf16 evaluation")
        off, tiles, self._layout, self._views = 0, 0, [], {}
        for c in self.convs:
            K, Cin, Cout = c.kernel_volume, c.in_channels, c.out_channels
            self._layout.append((off, K, Cin, Cout, tiles))
            off += K * Cin * Cout
            tiles += K * (Cin // 32) * (Cout // 32)
        self.total_tiles = tiles
        self.buf = torch.empty(off, dtype=torch.bfloat16, device=self.convs[0].kernel.device)
        for c, (o, K, Cin, Cout, _) in zip(self.convs, self._layout):
            self._views[c] = self.buf[o:o + K * Cin * Cout].view(K, Cout, Cin)
        self.packs = 0
        self.refresh()

    def refresh(self):
        """pack the weights as they are now (source offsets are taken afresh: an optimiser may have moved the parameters
        into its flat buffer since the last call)"""
        kernels = [c.kernel.detach() for c in self.convs]
        for k in kernels:
            if k.device != self.buf.device or k.dtype != torch.float32 or not k.is_contiguous():
                raise ValueError("Bf16Kernels: kernels must be contiguous float32 tensors on the table's device")
        base = kernels[0]
        desc = [((k.data_ptr() - base.data_ptr()) // 4, o, K, Cin, Cout, t)
                for k, (o, K, Cin, Cout, t) in zip(kernels, self._layout)]
        desc = torch.tensor(desc, dtype=torch.int64).to(self.buf.device)
        with torch.cuda.device(self.buf.device):
            call("lidog_pack_kernels_bf16", ptr(base), ptr(self.buf), ptr(desc), len(kernels), self.total_tiles)
        self.packs += 1

    def get(self, conv):
        """the packed kernel of `conv`, or None when it is not in the table"""
        return self._views.get(conv)


class Bf16Context:
    """what bf16_inference yields: the table and the routes the convolutions took while it was current"""

    def __init__(self, kernels):
        self.kernels = kernels
        self.launches = collections.Counter()       # route -> convolution calls
        self.routes = {}                            # convolution module -> set of routes

    def count(self, conv, route):
        self.launches[route] += 1
        self.routes.setdefault(conv, set()).add(route)


# the routes of Bf16Context.launches
OS_BN, GEMM_REDUCE_BN, GEMM_REDUCE, GEMM_DIRECT, FP32 = \
    "os_bn_bf16", "gemm_bf16+reduce_rows_bn", "gemm_bf16+reduce_rows", "gemm_bf16", "fp32"
BF16_ROUTES = (OS_BN, GEMM_REDUCE_BN, GEMM_REDUCE, GEMM_DIRECT)


def current():
    """the thread's current Bf16Context, or None"""
    return getattr(_state, "ctx", None)


@contextlib.contextmanager
def _set(ctx):
    prev = current()
    _state.ctx = ctx
    try:
        yield ctx
    finally:
        _state.ctx = prev


def bf16_inference(model, kernels=None):
    """Context manager: the eligible convolutions of `model` that run with autograd disabled inside it take the bf16
    kernels.  `kernels`: a Bf16Kernels of the model packed earlier (None: pack now).  Yields a Bf16Context."""
    return _set(Bf16Context(kernels if kernels is not None else Bf16Kernels(model)))


def fp32_inference():
    """Context manager: no table is current inside it, whatever the caller set"""
    return _set(None)


def scope(model, precision, kernels=None):
    """the context of an evaluation entry point's `precision` argument: None changes nothing, "fp32" suspends a current
    table, "bf16" makes `kernels` (or a fresh table) current"""
    mode = resolve(precision)
    if mode is None:
        return contextlib.nullcontext(current())
    return bf16_inference(model, kernels) if mode else fp32_inference()
