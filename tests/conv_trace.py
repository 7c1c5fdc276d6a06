"""Exact launch traces of the sparse convolution's Python layer (lidog_amd/me.py), taken on the CPU.

That layer only chooses entry points and their arguments, so it can be driven without a GPU: `me.call` / `me.call_on`
are replaced by recorders, `me.ptr` by a labeller and `me.require_gpu` by a no-op; two KernelMaps are built by hand from
seeded neighbour tables and handed out by a stub manager; real MinkowskiConvolution / MinkowskiConvolutionTranspose
modules and `conv_bn` then run on CPU tensors (no kernel runs: every result is uninitialised memory).  A case records
the list of [entry point, labelled arguments ...] in launch order and the precision context's `launches`.

    python tests/conv_trace.py OUT.json.gz       # write the traces of the lidog_amd that is first on the path

tests/golden/conv_dispatch_trace.json.gz holds the traces of the commit BEFORE the route choice was gathered into
me._conv_rows; tests/test_conv_dispatch_cpu.py compares today's with it.  Needs the built library for the host-side
tile, work-item and workspace arithmetic (as tests/test_hostprep_cpu.py does)."""
import contextlib
import gzip
import json
import os
import sys
import traceback

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "conv_dispatch_trace.json.gz")

N_FINE, N_COARSE = 300, 90
# name -> (module class, kernel size, stride, Cin, Cout, bias, rows in, map key in, rows out, map key out)
LAYERS = {
    "k3_32_64": ("conv", 3, 1, 32, 64, False, N_FINE, 1, N_FINE, 1),
    "k3_1_32_stem": ("conv", 3, 1, 1, 32, False, N_FINE, 1, N_FINE, 1),
    "k3_32_6": ("conv", 3, 1, 32, 6, False, N_FINE, 1, N_FINE, 1),
    "k3_32_1": ("conv", 3, 1, 32, 1, False, N_FINE, 1, N_FINE, 1),   # its data gradient has Cin = 1: never the stem kernel
    "k2s2_32_64": ("conv", 2, 2, 32, 64, False, N_FINE, 1, N_COARSE, 2),
    "k2s2t_64_32": ("tconv", 2, 2, 64, 32, False, N_COARSE, 2, N_FINE, 1),
    "k1_32_64_bias": ("conv", 1, 1, 32, 64, True, N_FINE, 1, N_FINE, 1),
    "k1_96_7_bias": ("conv", 1, 1, 96, 7, True, N_FINE, 1, N_FINE, 1),
}
TRAIN_MODES = ("conv", "conv_bn", "conv_bn_skip")
EVAL_MODES = ("conv_nograd", "conv_bn_eval", "conv_bn_eval_res")
OVERLAPS = {"lane2": (True, 2), "lane1": (True, 1), "inline": (False, 2)}


def _eligible(layer):
    return LAYERS[layer][3] % 32 == 0 and LAYERS[layer][4] % 32 == 0


def _symmetric_nbr(rng, n):
    """[27, n] neighbour table of a coordinate map onto itself: nbr[k][o] = i  <=>  nbr[26 - k][i] = o, one input row
    per (offset, output row) at most and the other way round, the centre offset the identity"""
    nbr = np.full((27, n), -1, dtype=np.int32)
    nbr[13] = np.arange(n)
    for k in range(13):
        outs = rng.permutation(n)[: int(rng.integers(n // 10, n // 2))]
        ins = rng.permutation(n)[: outs.size]
        nbr[k, outs] = ins
        nbr[26 - k, ins] = outs
    return nbr


def _k2s2_nbr(rng, n_fine, n_coarse):
    """[8, n_coarse] neighbour table of a k2 s2 map: every fine row in exactly one pair, no empty coarse row"""
    first = rng.integers(0, 8, n_coarse) * n_coarse + np.arange(n_coarse)
    rest = rng.permutation(np.setdiff1d(np.arange(8 * n_coarse), first))[: n_fine - n_coarse]
    nbr = np.full(8 * n_coarse, -1, dtype=np.int32)
    nbr[np.concatenate([first, rest])] = rng.permutation(n_fine)
    return nbr.reshape(8, n_coarse)


_NBR = {"sym": _symmetric_nbr(np.random.default_rng(11), N_FINE),
        "k2s2": _k2s2_nbr(np.random.default_rng(12), N_FINE, N_COARSE)}


def _kernel_map(me, nbr, n_in):
    """the KernelMap of a neighbour table, as lidog_kernel_map_pairs lays it out: pairs by offset, by output row inside
    an offset, and both position tables"""
    K, n_out = nbr.shape
    ks, outs = np.nonzero(nbr >= 0)                 # row-major: by offset, then by output row
    ins = nbr[ks, outs]
    k_off = np.concatenate([[0], np.cumsum(np.bincount(ks, minlength=K))]).astype(np.int64)
    pos_out = np.full((K, n_out), -1, dtype=np.int32)
    pos_in = np.full((K, n_in), -1, dtype=np.int32)
    pos_out[ks, outs] = pos_in[ks, ins] = np.arange(ks.size, dtype=np.int32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))     # noqa: E731
    return me.KernelMap(K, n_in, n_out, t(k_off), k_off.tolist(), t(ins.astype(np.int32)), t(outs.astype(np.int32)),
                        t(pos_out), t(pos_in), t(nbr))


class _CoordMapStub:
    def __init__(self, n):
        self.n = n


class _Manager:
    """what a convolution asks of its CoordinateManager: the maps of this case, made afresh (their lazily built tables
    are part of the trace)"""

    def __init__(self, me):
        self.me, self.trace = me, []
        self.maps = {1: _CoordMapStub(N_FINE), 2: _CoordMapStub(N_COARSE)}
        self.kmaps = {(1, 1, 3, 1): _kernel_map(me, _NBR["sym"], N_FINE),
                      (1, 2, 2, 1): _kernel_map(me, _NBR["k2s2"], N_FINE)}
        self.identity = {}

    def handover(self):
        pass

    def kernel_map(self, s_in, s_out, kernel_size, dilation=1):
        return self.kmaps[(s_in, s_out, kernel_size, dilation)]

    def identity_map(self, n):
        if n not in self.identity:
            self.identity[n] = self.me._IdentityMap(n, "cpu")
        return self.identity[n]


class _Table:
    """a precision.Bf16Kernels / Bf16Training of one convolution: packed operands that are never read"""

    def __init__(self, conv):
        K, Cin, Cout = conv.kernel_volume, conv.in_channels, conv.out_channels
        self.conv = conv
        self.fwd = torch.empty((K, Cout, Cin), dtype=torch.bfloat16)
        self.dgrad = torch.empty((K, Cin, Cout), dtype=torch.bfloat16)

    def get(self, conv):
        return self.fwd if conv is self.conv else None

    def pair(self, conv):
        return (self.fwd, self.dgrad) if conv is self.conv else None


class _SentinelGroup:
    """stands for a process group: MinkowskiSyncBatchNorm takes the sync route, and the trace of a case ends where the
    forward pass asks lidog_amd.comm for this group's transport"""


class Tracer:
    """per case: the launches, and the names of the live tensors `ptr` labels them with"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.launches, self.names, self.keep = [], {}, []

    def name(self, label, t):
        if t is not None:
            self.keep.append(t)                     # alive until the case ends: no other tensor gets this address
            self.names[t.data_ptr()] = label
        return t

    def ptr(self, t):
        if t is None:
            return None
        assert t.is_contiguous(), "lidog_amd kernels need contiguous tensors"
        label = self.names.get(t.data_ptr())
        return label if label is not None else \
            "tmp[%s]:%s" % (",".join(str(s) for s in t.shape), str(t.dtype).replace("torch.", ""))

    @staticmethod
    def _plain(a):
        if a is None or isinstance(a, (str, bool)):
            return a
        if isinstance(a, (int, np.integer)):
            return int(a)
        if isinstance(a, (float, np.floating)):
            return float(a)
        raise TypeError(f"unexpected launch argument {a!r}")

    def call(self, name, *args):
        self.launches.append([name] + [self._plain(a) for a in args])

    def call_on(self, raw_stream, name, *args):
        self.launches.append(["on_lane", name] + [self._plain(a) for a in args])


@contextlib.contextmanager
def patched(me, tracer, os_mode, overlap):
    """lidog_amd.me on the recorders, with the switches of one case"""
    saved = {k: getattr(me, k) for k in ("call", "call_on", "ptr", "require_gpu", "_SCONV_OS", "_WGRAD_FIT")}
    lane = (me._WgradLane.enabled, me._WgradLane.mode)
    sync_group = me.MinkowskiSyncBatchNorm._sync_group
    me.call, me.call_on, me.ptr, me.require_gpu = tracer.call, tracer.call_on, tracer.ptr, lambda t, what: None
    me._SCONV_OS = os_mode
    # work items cut by the pair count alone: fitting them to the kernel's slots asks the device for its CU count
    me._WGRAD_FIT = 0
    me.set_backward_overlap(*overlap)
    me.MinkowskiSyncBatchNorm._sync_group = lambda self: _SentinelGroup.instance
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(me, k, v)
        me._WgradLane.enabled, me._WgradLane.mode = lane
        me.MinkowskiSyncBatchNorm._sync_group = sync_group


_SentinelGroup.instance = _SentinelGroup()


def _stopped_at_the_collective(exc):
    """the exception came out of lidog_amd.comm.transport(group), called by the BatchNorm's forward pass"""
    frames = traceback.extract_tb(exc.__traceback__)
    return any(f.name == "transport" and f.filename.endswith(os.path.join("lidog_amd", "comm.py")) for f in frames)


def run_case(me, precision, tracer, layer, mode, prec, os_mode, overlap, sync=False):
    """{"launches": [...], "counts": {route: n} or None} of one case"""
    kind, ksize, stride, Cin, Cout, bias, n_in, key_in, n_out, key_out = LAYERS[layer]
    g = torch.Generator().manual_seed(5)
    tracer.reset()
    with patched(me, tracer, os_mode, overlap):
        cm = _Manager(me)
        cls = me.MinkowskiConvolution if kind == "conv" else me.MinkowskiConvolutionTranspose
        conv = cls(Cin, Cout, kernel_size=ksize, stride=stride, bias=bias, dimension=3)
        bnm = (me.MinkowskiSyncBatchNorm if sync else me.MinkowskiBatchNorm)(Cout)
        grad = mode in TRAIN_MODES
        conv.train(grad), bnm.train(grad)
        xf = torch.randn((n_in, Cin), generator=g).requires_grad_(grad)
        res = torch.randn((n_out, Cout), generator=g)
        tracer.name("x", xf), tracer.name("W", conv.kernel), tracer.name("bias", conv.bias), tracer.name("res", res)
        for label, t in (("bn.weight", bnm.bn.weight), ("bn.bias", bnm.bn.bias),
                         ("bn.running_mean", bnm.bn.running_mean), ("bn.running_var", bnm.bn.running_var)):
            tracer.name(label, t)
        m = {3: cm.kmaps[(1, 1, 3, 1)], 2: cm.kmaps[(1, 2, 2, 1)], 1: cm.identity_map(N_FINE)}[ksize]   # this layer's map
        if ksize > 1:
            for label in ("pair_in", "pair_out", "nbr", "k_off"):
                tracer.name(label, getattr(m, label))
            tracer.name("pos_in", m._pos_in), tracer.name("pos_out", m._pos_out)
        else:
            tracer.name("identity_rows", m.rows)
        for label, row in zip(("tile_k", "tile_row0", "tile_rows"), m.tiles):
            tracer.name(label, row)
        pctx = None
        if prec == "bf16":
            table = _Table(conv)
            tracer.name("wp_fwd", table.fwd), tracer.name("wp_dgrad", table.dgrad)
            pctx = (precision.Bf16TrainContext if grad else precision.Bf16Context)(table)
        x = me.SparseTensor(xf, coordinate_manager=cm, coordinate_map_key=key_in)
        residual = me.SparseTensor(res, coordinate_manager=cm, coordinate_map_key=key_out)
        stopped = None
        with precision._set(pctx), torch.set_grad_enabled(grad):
            try:
                if mode == "conv":
                    outs = [conv(x).F]
                elif mode == "conv_bn":
                    outs = [me.conv_bn(conv, bnm, x, relu=True).F]
                elif mode == "conv_bn_skip":
                    y, alias = me.conv_bn(conv, bnm, x, relu=True, skip=True)
                    outs = [y.F, alias.F]           # the residual branch's gradient comes back through the alias
                elif mode == "conv_nograd":
                    outs = [conv(x).F]
                elif mode == "conv_bn_eval":
                    outs = [me.conv_bn(conv, bnm, x, relu=True).F]
                else:
                    outs = [me.conv_bn(conv, bnm, x, relu=True, residual=residual).F]
                if grad:
                    tracer.launches.append(["-- backward --"])
                    grads = [tracer.name("gout" if i == 0 else "gskip", torch.randn(o.shape, generator=g))
                             for i, o in enumerate(outs)]
                    torch.autograd.backward(outs, grads)
            except Exception as exc:    # noqa: BLE001 -- a sync case ends at the collective, anything else is an error
                if not (sync and _stopped_at_the_collective(exc)):
                    raise
                stopped = "comm.transport"
        out = {"launches": tracer.launches, "counts": dict(sorted(pctx.launches.items())) if pctx is not None else None}
        if sync:
            out["stopped_at"] = stopped
    tracer.reset()
    return out


def cases():
    """(case id, arguments of run_case behind the tracer) of the whole matrix"""
    for os_mode in (0, 2):
        for layer in LAYERS:
            for prec in ("fp32", "bf16"):
                for mode in TRAIN_MODES + EVAL_MODES:
                    # under a context an ineligible layer only counts as fp32: pinned by the plain modes
                    if prec == "bf16" and not _eligible(layer) and mode not in ("conv", "conv_nograd"):
                        continue
                    for oname, overlap in OVERLAPS.items():
                        if oname != "lane2" and mode not in TRAIN_MODES:
                            continue
                        yield f"os{os_mode}/{layer}/{prec}/{mode}/{oname}", (layer, mode, prec, os_mode, overlap, False)
                    if mode in ("conv_bn", "conv_bn_skip"):
                        yield f"os{os_mode}/{layer}/{prec}/{mode}/sync", (layer, mode, prec, os_mode, OVERLAPS["lane2"], True)


def trace_all():
    """{case id: result of run_case} with the lidog_amd that `import lidog_amd` finds"""
    import lidog_amd.me as me
    from lidog_amd import precision
    tracer = Tracer()
    return {cid: run_case(me, precision, tracer, *args) for cid, args in cases()}


def dumps(launch):
    """one launch as text: 300 and 300.0, which compare equal, are different arguments"""
    return json.dumps(launch)


def load_golden(path=GOLDEN):
    with gzip.open(path, "rt") as f:
        return json.load(f)


def main(out):
    import lidog_amd
    traces = trace_all()
    print("traced", os.path.dirname(lidog_amd.__file__))
    data =json.dumps(traces, indent=0, sort_keys=True).encode()
    with open(out, "wb") as raw, gzip.GzipFile(filename="", fileobj=raw, mode="wb", mtime=0) as f:
        f.write(data)
    print(f"{len(traces)} cases, {sum(len(t['launches']) for t in traces.values())} launches, {len(data)} bytes of json "
          f"-> {out}")


if __name__ == "__main__":
    sys.path.append(REPO)       # behind PYTHONPATH: the package under trace may be another checkout's
    main(sys.argv[1])
