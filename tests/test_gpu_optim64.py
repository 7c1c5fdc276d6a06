"""The optimiser kernels (csrc/optim.hip k_adam / k_sgd) and the kernel transposes (csrc/sconv.hip k_transpose /
k_transpose_batched) through the C ABI against the float64 yardstick of tests/optim_ref.py, and the caching rule on top of
the transposes (optim.TransposedKernels: `p._wt_view` is read whenever `p._wt_version == p._version`).

Bars, none of them a tuned constant: every output of a step within adam_bounds / sgd_bounds (first-order fp32 error
propagation, derived in optim_ref; tests/test_optim_ref_cpu.py shows float32 torch.optim inside them and nine wrong
variants outside); on the model's own layout also within 2 x the distance of float32 CPU torch.optim from the same
yardstick, each implementation stepped from its own previous state; transposes and everything a launch must not touch:
bit equality.  The distance is the root mean square over a buffer of error / bound (the data span twelve decades: an
absolute norm would see the largest elements only).  Not the worst ratio: torch's CPU kernels fuse g + wd p and the
products of lerp / addcmul into one rounding where a chain built with -ffp-contract=off makes two of the same size, so a
correct kernel's worst ratio tends to exactly 2 x torch's on a first step (buf' = g': 1/3 against 1/6 of the bound) and
would sit on the bar, while two independent roundings for one give sqrt(2) in the mean square, which leaves the factor
2 its headroom (tests/test_optim_ref_cpu.py shows the numpy chain inside it).  Worst and rms ratios of both are recorded
with record_property.

The float64 side runs as torch float64 on the GPU (the same optim_ref expressions that run in numpy on the host)."""
import numpy as np
import pytest
import torch

import optim_ref as R
from helpers import small_batch

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, MU = 1e-2, 0.9, 0.999, 1e-8, 0.98
BAND = 64
CAP = 8192 * 256                       # elements one trip of the grid-stride loop covers
SIZES = [(1, 0), (255, 0), (256, 0), (257, 0), (CAP - 1, 0), (CAP + 257, 0), (4099, 1)]   # (n, odd lead)
MODEL_KW = dict(in_channels=1, out_channels=7, D=3, decoder_2d_level=["block8"], mapping_bound_2d=5.0)


def _lib():
    from lidog_amd import _lib as L
    return L.load(), L.stream


def _bits(t):
    return t.view(torch.int32)


class _Banded:
    """x [n] inside a larger buffer: `lead` floats, a guard band of 64 sentinel floats, x, another band.  lead = 0 puts x
    on a 256-byte boundary; an odd lead on an odd element (4-byte alignment only)."""

    def __init__(self, x, lead, salt):
        n = x.shape[0]
        self.lo, self.hi = lead + BAND, lead + BAND + n
        self.buf = (torch.arange(self.hi + BAND, dtype=torch.float32, device="cuda") * 0.5 + (1000.0 + salt))
        self.buf[self.lo:self.hi] = x
        self.before = self.buf.clone()

    @property
    def x(self):
        return self.buf[self.lo:self.hi]

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.lo

    def bands_untouched(self):
        return torch.equal(_bits(self.buf[:self.lo]), _bits(self.before[:self.lo])) and \
            torch.equal(_bits(self.buf[self.hi:]), _bits(self.before[self.hi:]))

    def untouched(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


def _banded(arrays, lead):
    """the odd leads differ per buffer (1, 3, 5, 7): no two slices share an alignment either"""
    return [_Banded(torch.from_numpy(a).cuda(), (lead + 2 * i) if lead else 0, 100 * i) for i, a in enumerate(arrays)]


def _record(record_property, worst):
    for k, r in worst.items():
        record_property(f"worst_error_over_bound_{k}", r)


# ------------------------------------------------------------------ Adam and SGD, one launch
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("s", [1.0, 0.25])
@pytest.mark.parametrize("step", [1, 7, 100000])
def test_adam_step_within_its_float32_bounds(step, s, wd, record_property):
    L, stream = _lib()
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for n, lead in SIZES:
        data = R.make_data(n, 3, wd, s)
        P, G, M, V = _banded(data, lead)
        if lead:
            assert all((b.ptr() % 16) != 0 and ((b.ptr() // 4) & 1) for b in (P, G, M, V))
        a = (LR, B1, B2, EPS, wd, step, s)
        dev = [b.x.clone() for b in (P, G, M, V)]
        ref, bounds = R.adam64(*dev, *a), R.adam_bounds(*dev, *a)
        if n >= 4096:
            share = R.small_denominator_share(ref[2].cpu().numpy(), B2, step, EPS)
            assert share >= 0.03, f"eps decides only {share:.3%} of the elements"
        rc = L.lidog_adam_step(P.ptr(), G.ptr(), M.ptr(), V.ptr(), n, LR, B1, B2, EPS, wd, step, s, stream())
        torch.cuda.synchronize()
        assert rc == 0
        what = f"n {n} lead {lead}"
        for k, b, r64, e in zip(("p", "m", "v"), (P, M, V), ref, bounds):
            r = R.worst_ratio(b.x, r64, e)
            print(f"adam step {step} s {s} wd {wd} {what}: {k} error / bound {r:.4f}")
            worst[k] = max(worst[k], r) if r == r else r
            assert b.bands_untouched(), f"{what}: guard band of {k} changed"
        assert G.untouched(), f"{what}: the gradient changed"
        for k in worst:
            assert worst[k] <= 1.0, f"{what}: {k} is {worst[k]:.3g} x its bound"
    _record(record_property, worst)


@pytest.mark.parametrize("s", [1.0, 0.25])
@pytest.mark.parametrize("nesterov,mu", [(1, MU), (0, MU), (0, 0.0)])
def test_sgd_step_within_its_float32_bounds(nesterov, mu, s, record_property):
    L, stream = _lib()
    wd = 1e-4
    worst = {"p": 0.0, "buf": 0.0}
    for n, lead in SIZES:
        p, g, m, _ = R.make_data(n, 3, wd, s)
        P, G, Bf = _banded((p, g, m), lead)
        a = (LR, mu, wd, nesterov, s)
        dev = [b.x.clone() for b in (P, G, Bf)]
        ref, bounds = R.sgd64(*dev, *a), R.sgd_bounds(*dev, *a)
        rc = L.lidog_sgd_step(P.ptr(), G.ptr(), Bf.ptr(), n, LR, mu, wd, nesterov, s, stream())
        torch.cuda.synchronize()
        assert rc == 0
        what = f"n {n} lead {lead}"
        for k, b, r64, e in zip(("p", "buf"), (P, Bf), ref, bounds):
            r = R.worst_ratio(b.x, r64, e)
            print(f"sgd nesterov {nesterov} mu {mu} s {s} {what}: {k} error / bound {r:.4f}")
            worst[k] = max(worst[k], r) if r == r else r
            assert b.bands_untouched(), f"{what}: guard band of {k} changed"
        assert G.untouched(), f"{what}: the gradient changed"
        for k in worst:
            assert worst[k] <= 1.0, f"{what}: {k} is {worst[k]:.3g} x its bound"
    _record(record_property, worst)


def test_empty_and_refused_steps_write_nothing():
    L, stream = _lib()
    bufs = _banded(R.make_data(300, 3), 0)
    P, G, M, V = bufs
    assert L.lidog_adam_step(P.ptr(), G.ptr(), M.ptr(), V.ptr(), 0, LR, B1, B2, EPS, 1e-4, 1, 1.0, stream()) == 0
    assert L.lidog_sgd_step(P.ptr(), G.ptr(), M.ptr(), 0, LR, MU, 1e-4, 1, 1.0, stream()) == 0
    assert L.lidog_sgd_step(P.ptr(), G.ptr(), M.ptr(), 300, -LR, MU, 1e-4, 1, 1.0, stream()) != 0
    assert L.lidog_sgd_step(P.ptr(), G.ptr(), M.ptr(), 300, LR, -MU, 1e-4, 1, 1.0, stream()) != 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in bufs)


# ------------------------------------------------------------------ a trajectory on the model's own layout
POOL = 1000003       # prime: the data maker's blocks meet every parameter at another offset


def _pool(seed, total, wd):
    """make_data of POOL elements repeated over `total` (a 37 M element draw takes numpy longer than the test may)"""
    idx = torch.arange(total, device="cuda") % POOL
    return [torch.from_numpy(a).cuda()[idx] for a in R.make_data(POOL, seed, wd, 1.0)]


def _yardstick_ratios(kind, pre, g, post, steps_el, hp):
    """worst error / bound per buffer of one step from `pre` to `post` (lists of float32 device tensors; Adam: p, m, v;
    SGD: p, buf), over the elements with steps_el > 0 (those that got a gradient), per distinct step count"""
    names = ("p", "m", "v") if kind == "Adam" else ("p", "buf")
    worst, sq, cnt = dict.fromkeys(names, 0.0), dict.fromkeys(names, 0.0), 0
    for st in sorted(set(steps_el.unique().tolist()) - {0}):
        idx = (steps_el == st).nonzero().squeeze(1)
        x = [t[idx] for t in pre]
        if kind == "Adam":
            a = (hp["lr"], B1, B2, EPS, hp["wd"], int(st), 1.0)
            ref, bounds = R.adam64(x[0], g[idx], x[1], x[2], *a), R.adam_bounds(x[0], g[idx], x[1], x[2], *a)
        else:
            a = (hp["lr"], MU, hp["wd"], 1, 1.0)
            ref, bounds = R.sgd64(x[0], g[idx], x[1], *a), R.sgd_bounds(x[0], g[idx], x[1], *a)
        for k, t, r64, e in zip(names, post, ref, bounds):
            r = R.worst_ratio(t[idx], r64, e)
            worst[k] = max(worst[k], r) if r == r else r
            sq[k] += R.ratio_square_sum(t[idx], r64, e)[0]
        cnt += idx.numel()
    return worst, {k: float(np.sqrt(sq[k] / max(cnt, 1))) for k in names}


@pytest.mark.parametrize("kind", ["Adam", "SGD"])
def test_two_steps_on_the_model_layout_against_float64_and_torch(kind, record_property):
    """FlatAdam / FlatSGD over MinkUNet34BEV, gradients written straight into flat.grad.  Step 1: `final.*` and every
    fifth parameter get none (torch skips them entirely: no decay, no moments, no step count); step 2: all get one."""
    import lidog_amd
    from lidog_amd.optim import FlatAdam, FlatSGD
    hp = dict(lr=LR, wd=1e-4)
    model = lidog_amd.MinkUNet34BEV(**MODEL_KW).cuda()
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    if kind == "Adam":
        opt = FlatAdam(model, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=hp["wd"])
        state = lambda: [opt.exp_avg, opt.exp_avg_sq]
    else:
        opt = FlatSGD(model, lr=LR, momentum=MU, weight_decay=hp["wd"], nesterov=True)
        state = lambda: [opt.momentum_buffer]
    flat = opt.flat
    sizes = [p.numel() for p in flat.params]
    flat.flat.copy_(_pool(3, flat.total, hp["wd"])[0])
    # the float32 CPU twin: torch.optim with the same float32 hyper-parameters widened to double
    twin = [torch.nn.Parameter(flat.flat[o:o + n].cpu().view(p.shape)) for p, o, n in zip(flat.params, flat.offsets, sizes)]
    tkw = dict(lr=R.f32(LR), weight_decay=R.f32(hp["wd"]), foreach=False)
    ref_opt = torch.optim.Adam(twin, betas=(R.f32(B1), R.f32(B2)), eps=R.f32(EPS), **tkw) if kind == "Adam" else \
        torch.optim.SGD(twin, momentum=R.f32(MU), nesterov=True, **tkw)
    tkeys = ("exp_avg", "exp_avg_sq") if kind == "Adam" else ("momentum_buffer",)

    def twin_flat():
        """the twin's parameters and state as flat device tensors (no state yet: zeros, as the flat buffers hold)"""
        out = [torch.cat([q.detach().reshape(-1) for q in twin]).cuda()]
        for k in tkeys:
            out.append(torch.cat([ref_opt.state[q][k].reshape(-1) if k in ref_opt.state.get(q, {})
                                  else torch.zeros(q.numel()) for q in twin]).cuda())
        return out

    expect = [0] * len(sizes)
    for it in (1, 2):
        g = _pool(3 if it == 1 else 40 + it, flat.total, hp["wd"])[1]
        skipped = [it == 1 and (name.startswith("final.") or i % 5 == 0) for i, name in enumerate(names)]
        assert it == 2 or (any(skipped) and not all(skipped))
        opt.zero_grad()
        flat.grad.copy_(g)
        g_cpu = g.cpu()
        for i, (p, q, off, n) in enumerate(zip(flat.params, twin, flat.offsets, sizes)):
            p.grad = None if skipped[i] else flat.grad[off:off + n].view(p.shape)
            q.grad = None if skipped[i] else g_cpu[off:off + n].view(q.shape)
            expect[i] += 0 if skipped[i] else 1
        steps_el = torch.repeat_interleave(torch.tensor([0 if sk else e for sk, e in zip(skipped, expect)]),
                                           torch.tensor(sizes)).cuda()
        pre = [t.clone() for t in [flat.flat] + state()]
        pre_twin = twin_flat()
        opt.step()
        ref_opt.step()
        torch.cuda.synchronize()
        post = [flat.flat] + state()
        assert torch.equal(_bits(flat.grad), _bits(g)), f"step {it}: the gradient buffer changed"
        still = steps_el == 0
        for t0, t1 in zip(pre, post):
            assert torch.equal(_bits(t0[still]), _bits(t1[still])), f"step {it}: a skipped slice changed"
        assert opt.param_steps == expect
        if kind == "Adam":
            assert [int(ref_opt.state[q]["step"]) if q in ref_opt.state else 0 for q in twin] == expect
        else:
            assert [int(q in ref_opt.state) for q in twin] == [min(e, 1) for e in expect]
        ours, ours_rms = _yardstick_ratios(kind, pre, g, post, steps_el, hp)
        theirs, theirs_rms = _yardstick_ratios(kind, pre_twin, g, twin_flat(), steps_el, hp)
        for k in ours:
            print(f"{kind} step {it} {k}: error / bound worst {ours[k]:.4f} rms {ours_rms[k]:.4f}; float32 torch.optim "
                  f"worst {theirs[k]:.4f} rms {theirs_rms[k]:.4f}")
            for name, val in (("kernel_worst", ours[k]), ("kernel_rms", ours_rms[k]), ("torch_float32_worst", theirs[k]),
                              ("torch_float32_rms", theirs_rms[k])):
                record_property(f"step{it}_{k}_{name}", val)
        for k in ours:
            assert ours[k] <= 1.0, f"step {it} {k}: {ours[k]:.3g} x its bound"
            assert ours_rms[k] <= 2 * theirs_rms[k], \
                f"step {it} {k}: rms error / bound {ours_rms[k]:.3g}, float32 torch.optim {theirs_rms[k]:.3g}"


# ------------------------------------------------------------------ lidog_transpose_kernel
SHAPES = R.NET_SHAPES + R.GENERIC_SHAPES


def _weights(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).cuda()


@pytest.mark.parametrize("K,Cin,Cout", SHAPES)
def test_transpose_kernel_is_exact(K, Cin, Cout):
    from lidog_amd._lib import call, ptr
    W = _weights((K, Cin, Cout), K * 1000 + Cin)
    W0 = W.clone()
    n = W.numel()
    dst = torch.full((BAND + n + BAND,), float("nan"), device="cuda")
    call("lidog_transpose_kernel", ptr(W), K, Cin, Cout, dst.data_ptr() + 4 * BAND)
    torch.cuda.synchronize()
    assert torch.equal(dst[BAND:BAND + n].view(K, Cout, Cin), R.transpose64(W0).contiguous())
    assert bool(dst[:BAND].isnan().all()) and bool(dst[BAND + n:].isnan().all()), "written outside the destination"
    assert torch.equal(W, W0)


# ------------------------------------------------------------------ lidog_transpose_batched
# full-tile and ragged matrices alternate; the table's first-tile column is what the kernel's binary search reads.  With a
# 7-float gap in the source and a 1-float gap in the destination before every matrix, the k-th matrix (from 1) starts at
# S + 7k and S + k floats (S: the sizes before it); both are multiples of 4 only for even k, where the ragged ones sit
TABLE = [SHAPES[i] for i in (1, 8, 5, 9, 2, 0, 3, 10, 4, 6, 7, 11)]


def _table(shapes, src_gap, dst_gap, align):
    """(desc rows, src length, dst length): every matrix preceded by its gap, offsets then rounded up to `align` floats"""
    rows, so, do, tiles = [], 0, 0, 0
    up = lambda x: -(-x // align) * align
    for K, Cin, Cout in shapes:
        so, do = up(so + src_gap), up(do + dst_gap)
        rows.append((so, do, K, Cin, Cout, tiles))
        so, do = so + K * Cin * Cout, do + K * Cin * Cout
        tiles += K * (-(-Cin // 32)) * (-(-Cout // 32))
    return rows, so, do, tiles


def _run_batched(shapes, src_gap, dst_gap, align):
    from lidog_amd._lib import call, ptr
    rows, n_src, n_dst, tiles = _table(shapes, src_gap, dst_gap, align)
    src = _weights((n_src + BAND,), 17 + src_gap)
    src0 = src.clone()
    dst = torch.full((n_dst + BAND,), float("nan"), device="cuda")
    desc = torch.tensor(rows, dtype=torch.int64, device="cuda").view(-1, 6)
    call("lidog_transpose_batched", ptr(src), ptr(dst), ptr(desc), len(rows), tiles)
    torch.cuda.synchronize()
    written = torch.zeros(n_dst + BAND, dtype=torch.bool, device="cuda")
    for so, do, K, Cin, Cout, _ in rows:
        n = K * Cin * Cout
        want = R.transpose64(src0[so:so + n].view(K, Cin, Cout)).contiguous()
        assert torch.equal(dst[do:do + n].view(K, Cout, Cin), want), f"matrix {(K, Cin, Cout)} at {so} -> {do}"
        written[do:do + n] = True
    assert bool(dst[~written].isnan().all()), "a gap or the tail of the destination was written"
    assert int((~written).sum()) >= BAND
    assert torch.equal(src, src0)
    return rows, src, dst


def test_transpose_batched_on_aligned_offsets():
    rows, src, dst = _run_batched(TABLE, 0, 0, 4)
    for so, do, K, Cin, Cout, _ in rows:      # the 32-multiple shapes qualify for the 16-byte path
        assert (src.data_ptr() + 4 * so) % 16 == 0 and (dst.data_ptr() + 4 * do) % 16 == 0


def test_transpose_batched_on_unaligned_offsets():
    rows, src, dst = _run_batched(TABLE, 7, 1, 1)
    full = [(so, do) for so, do, K, Cin, Cout, _ in rows if Cin % 32 == 0 and Cout % 32 == 0]
    assert len(full) == 6
    for so, do in full:                       # none of them does here: same shapes, scalar path
        assert ((src.data_ptr() + 4 * so) | (dst.data_ptr() + 4 * do)) % 16 != 0


def test_transpose_batched_one_matrix_and_none():
    from lidog_amd._lib import call, ptr
    _run_batched([(27, 96, 96)], 0, 0, 4)
    _run_batched([(2, 33, 31)], 7, 1, 1)
    src = _weights((256,), 5)
    dst = torch.full((256,), float("nan"), device="cuda")
    desc = torch.tensor([(0, 0, 1, 16, 16, 0)], dtype=torch.int64, device="cuda")
    call("lidog_transpose_batched", ptr(src), ptr(dst), ptr(desc), 0, 1)
    call("lidog_transpose_batched", ptr(src), ptr(dst), None, 0, 0)
    torch.cuda.synchronize()
    assert bool(dst.isnan().all())


# ------------------------------------------------------------------ TransposedKernels: is the cached copy fresh?
def _kernels(model):
    return [(n, p) for n, p in model.named_parameters() if getattr(p, "_lidog_sparse_kernel", False)]


def _fresh(model):
    """every kernel: either its copy is marked stale (backward transposes per layer) or it IS the transpose of the
    current weights; returns how many copies are marked current"""
    current = 0
    for name, p in _kernels(model):
        if p._wt_version != p._version:
            continue
        current += 1
        w = p.detach() if p.dim() == 3 else p.detach().unsqueeze(0)
        assert torch.equal(p._wt_view, R.transpose64(w).contiguous()), f"{name}: stale transposed copy marked current"
    return current


def _random_grads(opt, seed):
    opt.zero_grad()
    g = torch.Generator(device="cuda").manual_seed(seed)
    opt.flat.grad.copy_(torch.randn(opt.flat.total, device="cuda", generator=g) * 1e-2)
    for p, off in zip(opt.flat.params, opt.flat.offsets):
        p.grad = opt.flat.grad[off:off + p.numel()].view(p.shape)


@pytest.mark.parametrize("kind", ["Adam", "SGD"])
def test_transposed_kernels_are_fresh_or_marked_stale(kind):
    import lidog_amd
    import lidog_amd.me as ME
    from lidog_amd.optim import make_optimizer
    model = lidog_amd.MinkUNet34BEV(**MODEL_KW).cuda()
    convs = [m for m in model.modules() if isinstance(m, (ME.MinkowskiConvolution, ME.MinkowskiConvolutionTranspose))]
    opt = make_optimizer(kind, model, 1e-2)
    n = len(convs)
    assert n == 63 and len(_kernels(model)) == n == len(opt.transposed.items)
    assert opt.transposed.buf.numel() == sum(m.kernel.numel() for m in convs)
    assert _fresh(model) == n, "after construction"
    for it in range(2):
        _random_grads(opt, it)
        w0 = opt.flat.flat.clone()
        opt.step()
        assert not torch.equal(w0, opt.flat.flat)
        assert _fresh(model) == n, f"after step {it}"
    other = {k: (v * 1.5 + 0.01 if v.is_floating_point() else v.clone()) for k, v in model.state_dict().items()}
    for layout in ("flat", "torch"):
        sd = opt.state_dict() if layout == "flat" else opt.torch_state_dict()
        model.load_state_dict(other)            # alone: every copy is now stale, and must say so
        assert _fresh(model) == 0, "after model.load_state_dict: a stale copy is still marked current"
        opt.load_state_dict(sd)
        assert _fresh(model) == n, f"after opt.load_state_dict ({layout} layout)"
        other = {k: (v * 0.5 if v.is_floating_point() else v.clone()) for k, v in other.items()}
    name, p = _kernels(model)[7]
    with torch.no_grad():
        p.mul_(2)
    assert _fresh(model) == n - 1 and p._wt_version != p._version, f"after an in-place edit of {name}"

    # the data gradients read the copy: one optimiser step, then the same backward from the copy and per layer
    _random_grads(opt, 9)
    opt.step()
    assert _fresh(model) == n
    coords = small_batch((0, 1), n_points=2500).cuda()
    cm = ME.SparseTensor(coordinates=coords, features=torch.ones((coords.shape[0], 1), device="cuda")).coordinate_manager
    for s_in, s_out in ((1, 2), (2, 4), (4, 8)):
        cm.stride(s_in, s_out)
    for conv, key, shape in ((model.block8[1].conv1, 1, (27, 96, 96)), (model.convtr5p8s2, 8, (8, 256, 128))):
        w = conv.kernel
        assert tuple(w.shape) == shape and w._wt_version == w._version
        rows = cm.maps[key].n
        g = torch.Generator().manual_seed(key)
        x0 = torch.randn(rows, shape[1], generator=g).cuda()
        w.requires_grad_(False)                 # the data gradient alone
        grads = []
        for per_layer in (False, True):
            version = w._wt_version
            if per_layer:
                w._wt_version = -1
            x = x0.clone().requires_grad_(True)
            y = conv(ME.SparseTensor(x, coordinate_manager=cm, coordinate_map_key=key)).F
            if not grads:
                gy = torch.randn(y.shape, generator=g).cuda()
            y.backward(gy)
            grads.append(x.grad.clone())
            w._wt_version = version
        w.requires_grad_(True)
        assert bool(grads[0].abs().sum() > 0) and torch.equal(grads[0], grads[1]), \
            f"{shape}: the data gradient from the cached copy differs from the per-layer transpose"
