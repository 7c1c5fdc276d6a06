"""Opt-in bf16: the sparse convolutions of evaluation passes, or of whole training steps, on the bf16 matrix instruction.

The reference passes `pipeline.precision` to Lightning's Trainer.  Here only the two operands of the matrix instruction
are bf16: activations, gradients, master weights, the flat gradient buffer and the optimiser state stay fp32 in memory
(every BatchNorm, residual, ReLU, concatenation, instance-norm, loss and metric kernel and the 2-D BEV head are
untouched); a convolution whose channel counts are multiples of 32 multiplies bf16 operands with fp32 accumulation
(csrc/sconv_bf16.hip): gathered rows are rounded as they are staged, the weights are packed.  No loss scaling: bf16 has
fp32's exponent range.

Evaluation (autograd disabled):

    with bf16_inference(model) as ctx:            # packs; or bf16_inference(model, kernels) with a Bf16Kernels
        preds, logits = evaluate.predict(model, coords, feats)
    ctx.launches                                  # Counter: route -> convolutions that took it

Training (autograd enabled; Fit(precision="bf16"), train --precision bf16, or a step class's precision="bf16"):

    table = Bf16Training(model)                   # after the optimiser was built: it reads its transposed kernels
    with bf16_training(model, table) as ctx:
        loss = ...; loss.backward()               # forward, data gradient and weight gradient of the eligible convolutions
    opt.step(); table.refresh()                   # what _Step.training_step does

Inside a training context the trunk executor declines (it launches the fp32 kernels from C) and the step goes down the
operator path; everything returns to it when the context exits.

A packed table is a SNAPSHOT of the weights.  Its validity is not tied to the parameters' version counters: the
optimiser's HIP kernels write through raw pointers and never advance them.  Whoever owns a table calls refresh() after
the weights change; a Bf16Training also notices, when it becomes current, that the optimiser's transposed copy it reads
was refreshed behind its back (load_state_dict, resume) and packs again.  Without a current table (the default) no code
path changes."""
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


def table_layout(shapes, off=0, tiles=0):
    """([(dst offset in bf16 elements, K, Cin, Cout, first 32 x 32 tile)] of kernels fp32 [K, Cin, Cout] packed back to
    back from element `off` and tile `tiles` on, end offset, end tile): the last five columns of a descriptor row of
    lidog_pack_kernels_bf16"""
    layout = []
    for K, Cin, Cout in shapes:
        layout.append((off, K, Cin, Cout, tiles))
        off += K * Cin * Cout
        tiles += K * (Cin // 32) * (Cout // 32)
    return layout, off, tiles


def training_layout(shapes):
    """(forward layout, data-gradient layout, elements, tiles) of a Bf16Training over kernels [K, Cin, Cout]: the
    forward operands first, then the packs of the transposed kernels [K, Cout, Cin] (source `Cin` = Cout), in one
    buffer and one tile range, so that ONE launch writes both"""
    fwd, off, tiles = table_layout(shapes)
    dgrad, off, tiles = table_layout([(K, Cout, Cin) for K, Cin, Cout in shapes], off, tiles)
    return fwd, dgrad, off, tiles


def _eligible_convs(model, what):
    convs = [m for m in model.modules() if eligible(m)]
    if not convs:
        raise ValueError(f"{what}: the model has no convolution with channel counts that are multiples of 32")
    for c in convs:
        require_gpu(c.kernel, f"the model of {what}")
    return convs


def _pack(base, buf, sources, layout, total_tiles, what):
    """one launch of lidog_pack_kernels_bf16: sources[i] (fp32, contiguous) -> layout[i] of buf; source offsets are taken
    afresh (an optimiser may have moved the parameters into its flat buffer since the last call)"""
    for k in sources:
        if k.device != buf.device or k.dtype != torch.float32 or not k.is_contiguous():
            raise ValueError(f"{what}: kernels must be contiguous float32 tensors on the table's device")
    desc = [((k.data_ptr() - base.data_ptr()) // 4,) + tuple(row) for k, row in zip(sources, layout)]
    desc = torch.tensor(desc, dtype=torch.int64).to(buf.device)
    with torch.cuda.device(buf.device):
        call("lidog_pack_kernels_bf16", ptr(base), ptr(buf), ptr(desc), len(sources), total_tiles)


class Bf16Kernels:
    """bf16 [K, Cout, Cin] copies of the kernels [K, Cin, Cout] of every eligible convolution of `model` (transposed:
    a lane's eight k-values of the B operand are 16 contiguous bytes), written by ONE launch of lidog_pack_kernels_bf16
    on construction and on every refresh()."""
    what, dgrad = "a bf16 evaluation", False    # Bf16Training: the data-gradient operands behind the forward ones

    def __init__(self, model):
        self.convs = _eligible_convs(model, self.what)
        shapes = [(c.kernel_volume, c.in_channels, c.out_channels) for c in self.convs]
        if not self.dgrad:
            self._layout, off, self.total_tiles = table_layout(shapes)
        else:
            owners = {id(getattr(c.kernel, "_wt_owner", None)) for c in self.convs}
            self.transposed = getattr(self.convs[0].kernel, "_wt_owner", None)
            if self.transposed is None or len(owners) != 1:
                raise ValueError("Bf16Training: build the model's optimiser first (the data-gradient table is packed "
                                 "from the transposed kernels it keeps, optim.TransposedKernels)")
            fwd, dgrad, off, self.total_tiles = training_layout(shapes)
            self._layout = fwd + dgrad
        self.buf = torch.empty(off, dtype=torch.bfloat16, device=self.convs[0].kernel.device)
        # a layout row's view is [K, its Cout, its Cin]: [K, Cout, Cin] forward, [K, Cin, Cout] for the data gradient
        views = [self.buf[o:o + K * Cin * Cout].view(K, Cout, Cin) for o, K, Cin, Cout, _ in self._layout]
        self._views = {c: tuple(views[i::len(self.convs)]) for i, c in enumerate(self.convs)}
        self.packs = 0
        self.refresh()

    def refresh(self):
        """pack the weights (Bf16Training: and their transposed copies) as they are now"""
        sources = [c.kernel.detach() for c in self.convs]
        if self.dgrad:
            sources += [c.kernel._wt_view for c in self.convs]
            self._seen = self.transposed.generation
        _pack(sources[0], self.buf, sources, self._layout, self.total_tiles, type(self).__name__)
        self.packs += 1

    def get(self, conv):
        """the packed kernel of `conv` -- the forward operand, also what a no_grad call inside a training context
        takes -- or None when it is not in the table"""
        views = self._views.get(conv)
        return views[0] if views is not None else None


class Bf16Training(Bf16Kernels):
    """The two bf16 operand tables of a mixed-precision training step over the eligible convolutions of `model`:
    forward   [K, Cout, Cin]: the pack of the kernel W [K, Cin, Cout], as Bf16Kernels;
    dgrad     [K, Cin, Cout]: the pack of the transposed kernel [K, Cout, Cin] that optim.TransposedKernels keeps for the
              fp32 data gradient (the B operand of the gathered GEMM over the exchanged map).
    Both are written by ONE launch of lidog_pack_kernels_bf16 (one descriptor table, source offsets relative to the
    first kernel).  The model's optimiser must exist: the table reads its transposed copy, so refresh() belongs AFTER
    TransposedKernels.refresh() -- i.e. after every optimiser step (_Step.training_step does that), and after
    load_state_dict / resume, which refresh the transposed copy: stale() sees that and bf16_training packs again."""
    what, dgrad = "bf16 training", True

    def stale(self):
        """the transposed copy was refreshed since the last pack (the weights were loaded or stepped without refresh())"""
        return self._seen != self.transposed.generation

    def pair(self, conv):
        """(forward operand, data-gradient operand) of `conv`, or None when it is not in the table"""
        return self._views.get(conv)


class Bf16Context:
    """what bf16_inference yields: the table and the routes the convolutions took while it was current"""
    training = False

    def __init__(self, kernels):
        self.kernels = kernels
        self.launches = collections.Counter()       # route -> convolution calls
        self.routes = {}                            # convolution module -> set of routes

    def count(self, conv, route):
        self.launches[route] += 1
        self.routes.setdefault(conv, set()).add(route)


class Bf16TrainContext(Bf16Context):
    """what bf16_training yields: `kernels` is a Bf16Training; grad-enabled calls of the eligible convolutions take the
    bf16 forward, data-gradient and weight-gradient kernels (the backward pass counts on the context its forward saw)"""
    training = True


# the routes of Bf16Context.launches
OS_BN, GEMM_REDUCE_BN, GEMM_REDUCE, GEMM_DIRECT, FP32 = \
    "os_bn_bf16", "gemm_bf16+reduce_rows_bn", "gemm_bf16+reduce_rows", "gemm_bf16", "fp32"
BF16_ROUTES = (OS_BN, GEMM_REDUCE_BN, GEMM_REDUCE, GEMM_DIRECT)
# grad-enabled calls under a Bf16TrainContext (an fp32 convolution is counted once, as FP32, by its forward pass)
FWD_DIRECT, FWD_REDUCE, DGRAD_DIRECT, DGRAD_REDUCE, WGRAD = \
    "fwd:gemm_bf16", "fwd:gemm_bf16+reduce_rows", "dgrad:gemm_bf16", "dgrad:gemm_bf16+reduce_rows", "wgrad:wgrad_bf16"
TRAIN_FWD_ROUTES, TRAIN_DGRAD_ROUTES = (FWD_DIRECT, FWD_REDUCE), (DGRAD_DIRECT, DGRAD_REDUCE)


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


def bf16_training(model, table=None):
    """Context manager: grad-enabled calls of the eligible convolutions of `model` inside it run forward, data gradient
    and weight gradient on the bf16 kernels, and the trunk executor declines.  `table`: a Bf16Training of the model (None:
    pack now); one that went stale is packed again first.  Yields a Bf16TrainContext."""
    if table is None:
        table = Bf16Training(model)
    elif table.stale():
        table.refresh()
    return _set(Bf16TrainContext(table))


def check_single_rank(what="precision='bf16' training"):
    """bf16 training steps go down the operator path; with more than one rank that is the SyncBatchNorm operator path,
    which is not validated in this mode"""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(
            f"{what} with {dist.get_world_size()} ranks: a bf16 step leaves the trunk executor for the operator path, "
            "and multi-rank training waits for the executor follow-up (csrc/trunk.hip learning the bf16 kernels)")


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
