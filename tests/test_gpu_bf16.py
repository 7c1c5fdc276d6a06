"""The opt-in bf16 inference path on the GPU (csrc/sconv_bf16.hip, lidog_amd/precision.py): the weight pack bit for bit,
the gathered GEMM and the output-stationary form against the float64 yardstick of tests/sconv_ref.py, poisoned rows, the
models' routes and logits, and TargetEvaluator end to end.

The reference of the two convolution kernels is sconv_ref.conv64 over the operands ROUNDED TO BF16 FIRST
(t.bfloat16().float(), round to nearest even: tests/test_bf16_cpu.py).  A product of two bf16 numbers is exact in fp32,
so what separates the kernels from that reference is fp32 accumulation alone, and the bar is 2 * sconv_ref.bound of the
rounded operands: derived, not measured; the factor 2 allows every accumulation inside the matrix unit an error of 2u
instead of u (an adder that truncates).  A kernel that truncated its operands instead of rounding them would be off by
2^-8 relative per operand, three orders of magnitude above that bar.

Outputs and product rows are pre-filled with NaN: a row left unwritten fails."""
import numpy as np
import pytest
import torch

import sconv_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
TIES = (0.0, -0.0, 1 + 2.0 ** -8, 1 + 2.0 ** -7 + 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 2.0 ** -7 + 2.0 ** -8))
GEMM_SCENES = ("tiny_1", "tiny_127", "tiny_128", "tiny_129", "line_x129", "dense_cube", "isolated", "twin_scans")
GEMM_KINDS = ("k3s1", "k2s2", "k3s2", "tr_k2s2", "identity")
GEMM_SHAPES = ((32, 32), (64, 64), (96, 96), (128, 96), (384, 256))
OS_SCENES = ("dense_cube", "line_x129", "isolated", "twin_scans", "tiny_129")
OS_SHAPES = ((32, 32), (96, 96), (128, 96))
_CMS = {}


def _map(name, kind):
    """the device kernel map of a map kind on one coordinate manager per scene"""
    import lidog_amd.me as ME
    if name not in _CMS:
        c = torch.from_numpy(R.scene(name)).cuda()
        _CMS[name] = ME.SparseTensor(coordinates=c, features=torch.ones((c.shape[0], 1), device="cuda")).coordinate_manager
    ks, stride, dil, _ = R.KINDS[kind]
    return _CMS[name].kernel_map(1, stride, ks, dil)


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _dev(t):
    """every float operand the tests own"""
    return t.cuda()


def _bf(t):
    """the operand as the kernels see it: rounded to bf16 (nearest even), back in float32"""
    return t.bfloat16().float()


def _operands(n_in, K, Cin, Cout, seed):
    g = torch.Generator().manual_seed(seed)
    x = _dev(torch.randn(n_in, Cin, generator=g))
    W = _dev(torch.randn(K, Cin, Cout, generator=g) * 0.1)
    b = _dev(torch.randn(Cout, generator=g))
    return x, W, b


def _pack(*kernels):
    """lidog_pack_kernels_bf16 over a table of [K, Cin, Cout] kernels, ONE call; the packed [K, Cout, Cin] views.  The
    sources are separate allocations (offsets of either sign from the first), the destination is pre-filled with the
    bf16 NaN pattern."""
    from lidog_amd._lib import call, ptr
    desc, off, tiles = [], 0, 0
    for W in kernels:
        K, Cin, Cout = W.shape
        assert W.is_contiguous() and (W.data_ptr() - kernels[0].data_ptr()) % 4 == 0
        desc.append(((W.data_ptr() - kernels[0].data_ptr()) // 4, off, K, Cin, Cout, tiles))
        off += W.numel()
        tiles += K * (-(-Cin // 32)) * (-(-Cout // 32))
    buf = _nan(off, dtype=torch.bfloat16)
    call("lidog_pack_kernels_bf16", ptr(kernels[0]), ptr(buf), ptr(torch.tensor(desc, dtype=torch.int64).cuda()),
         len(kernels), tiles)
    return [buf[d[1]:d[1] + W.numel()].view(W.shape[0], W.shape[2], W.shape[1]) for d, W in zip(desc, kernels)]


def _inside(got, ref, bnd, what):
    assert bool(torch.isfinite(got).all()), f"{what}: a row was left unwritten (NaN) or is not finite"
    r = R.worst_ratio(got, ref, bnd)
    print(f"{what}: error / bound {r:.3g}")
    assert r <= 1.0, f"{what}: error / bound {r:.3g}"
    return r


# ------------------------------------------------------------------ pack
def test_pack_is_bit_equal_to_torch_rounding():
    shapes = ((27, 32, 32), (8, 128, 96), (1, 96, 32), (27, 384, 256))
    g = torch.Generator().manual_seed(3)
    kernels = []
    for K, Cin, Cout in shapes:
        W = torch.randn(K, Cin, Cout, generator=g) * 0.1
        flat = W.view(-1)
        flat[:len(TIES)] = torch.tensor(TIES)                      # +-0 and the ties of tests/test_bf16_cpu.py
        flat[-len(TIES):] = torch.tensor(TIES) * 2.0 ** -20
        W[K - 1, Cin - 1, :len(TIES)] = torch.tensor(TIES) * 2.0 ** 10
        kernels.append(_dev(W))
    packed = _pack(*kernels)
    for W, Wp in zip(kernels, packed):
        want = W.transpose(1, 2).contiguous().bfloat16()
        assert Wp.shape == want.shape and Wp.dtype == torch.bfloat16
        assert torch.equal(Wp.view(torch.int16), want.view(torch.int16)), tuple(W.shape)
    first = packed[0].view(torch.int16)
    assert first[0, 0, 0].item() == 0 and first[0, 1, 0].item() == -32768      # W[0, 0, 0] = +0, W[0, 0, 1] = -0
    assert _bf(kernels[0])[0, 0, 2].item() == 1.0 and _bf(kernels[0])[0, 0, 3].item() == 1 + 2.0 ** -6


# ------------------------------------------------------------------ gathered GEMM
def _gemm_bf16(x, gather, Wp, bias, m, Cin, Cout, out, scatter):
    from lidog_amd._lib import call, ptr
    call("lidog_sconv_gemm_bf16", ptr(x), ptr(gather), ptr(Wp), ptr(bias), ptr(m.tiles[0]), ptr(m.tiles[1]),
         ptr(m.tiles[2]), m.n_tiles, Cin, Cout, ptr(out), ptr(scatter))


def _conv_two_pass(kind, name, x, Wp, b, Cin, Cout):
    """(output [n_out, Cout], product rows or None) of one map kind through lidog_sconv_gemm_bf16: the strided and
    same-stride kinds via product rows + lidog_sconv_reduce_rows, the transposed k2 s2 kind scattered straight into the
    output, the identity kind (no gather index) written in place"""
    import lidog_amd.me as ME
    from lidog_amd._lib import call, ptr
    if kind == "identity":
        n = x.shape[0]
        out = _nan(n, Cout)
        _gemm_bf16(x, None, Wp, b, ME._IdentityMap(n, "cuda"), Cin, Cout, out, None)
        return out, None
    if kind == "tr_k2s2":
        m = _map(name, "k2s2")
        out = _nan(m.n_in, Cout)
        _gemm_bf16(x, m.pair_out, Wp, b, m, Cin, Cout, out, m.pair_in)
        return out, None
    m = _map(name, kind)
    T = _nan(m.P, Cout)
    _gemm_bf16(x, m.pair_in, Wp, None, m, Cin, Cout, T, None)
    rp, rl = m.rows("out")
    out = _nan(m.n_out, Cout)
    call("lidog_sconv_reduce_rows", ptr(T), ptr(rp), ptr(rl), m.n_out, Cout, ptr(b), None, ptr(out))
    return out, T


def _nbr(name, kind):
    """(rows of the input, neighbour table [K, n_out]) of a kind"""
    if kind == "identity":
        n = R.scene(name).shape[0]
        return n, np.arange(n, dtype=np.int64)[None, :]
    cin, _, nbr = R.scene_map(name, kind)
    return cin.shape[0], nbr


@pytest.mark.parametrize("Cin,Cout", GEMM_SHAPES, ids=[f"{a}x{b}" for a, b in GEMM_SHAPES])
@pytest.mark.parametrize("name", GEMM_SCENES)
def test_gathered_gemm_against_float64_of_the_rounded_operands(name, Cin, Cout, record_property):
    """lidog_sconv_gemm_bf16 (+ lidog_sconv_reduce_rows) for every map kind, with and without bias, inside
    2 * sconv_ref.bound of the bf16-rounded operands.  Observed worst error / bound over all cases on MI355X: 0.022
    (DESIGN.md section 3r)."""
    worst = 0.0
    for kind in GEMM_KINDS:
        n_in, nbr = _nbr(name, kind)
        x, W, b = _operands(n_in, nbr.shape[0], Cin, Cout, Cin * 131 + Cout + len(kind))
        (Wp,) = _pack(W)
        xb, Wb = _bf(x), _bf(W)
        for bias in (b, None):
            y, _ = _conv_two_pass(kind, name, x, Wp, bias, Cin, Cout)
            ref, bnd = R.conv64(xb, Wb, bias, nbr), 2 * R.bound(xb, Wb, bias, nbr)
            assert y.shape == ref.shape
            worst = max(worst, _inside(y, ref, bnd, f"{name} {kind} {Cin}->{Cout} bias {bias is not None}"))
    record_property("worst_error_over_bound", worst)


# ------------------------------------------------------------------ output-stationary form
class Os:
    """one 3^3 convolution + evaluation-mode BatchNorm through both bf16 routes"""

    def __init__(self, name, Cin, Cout):
        from test_gpu_sconv_os import _sorted
        self.name, self.Cin, self.Cout = name, Cin, Cout
        self.m = _map(name, "k3s1")
        self.n = self.m.n_out
        self.nbr = R.scene_map(name, "k3s1")[2]
        self.x, self.W, self.b = _operands(self.n, 27, Cin, Cout, Cin * 977 + Cout)
        (self.Wp,) = _pack(self.W)
        self.sorted = _sorted(self.m)
        g = torch.Generator().manual_seed(Cin + 7 * Cout)
        self.bn = tuple(_dev(v) for v in (torch.randn(Cout, generator=g) * 0.3, torch.rand(Cout, generator=g) + 0.5,
                                          torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.3))
        self.res = _dev(torch.randn(self.n, Cout, generator=g))      # mean, invstd, weight, bias; residual

    def os_bn(self, x, residual, relu):
        from lidog_amd._lib import call, ptr
        perm, wm, order = self.sorted
        out = _nan(self.n, self.Cout)
        call("lidog_sconv_os_bn_bf16", ptr(x), ptr(self.m.nbr), self.n, 27, ptr(perm), ptr(wm), ptr(order), ptr(self.Wp),
             ptr(self.b), self.Cin, self.Cout, *(ptr(v) for v in self.bn), ptr(residual), relu, ptr(out))
        return out

    def product(self, x):
        T = _nan(self.m.P, self.Cout)
        _gemm_bf16(x, self.m.pair_in, self.Wp, None, self.m, self.Cin, self.Cout, T, None)
        return T

    def two_pass_bn(self, x, residual, relu):
        from lidog_amd._lib import call, ptr
        rp, rl = self.m.rows("out")
        out = _nan(self.n, self.Cout)
        call("lidog_sconv_reduce_rows_bn", ptr(self.product(x)), ptr(rp), ptr(rl), self.n, self.Cout, ptr(self.b),
             *(ptr(v) for v in self.bn), ptr(residual), relu, ptr(out))
        return out


@pytest.mark.parametrize("Cin,Cout", OS_SHAPES, ids=[f"{a}x{b}" for a, b in OS_SHAPES])
@pytest.mark.parametrize("name", OS_SCENES)
def test_output_stationary_form_against_float64(name, Cin, Cout, record_property):
    """lidog_sconv_os_bn_bf16, and lidog_sconv_gemm_bf16 + lidog_sconv_reduce_rows_bn, residual and ReLU on and off,
    against float64 of y = relu(((c - mean) invstd) w + b + residual) with c the convolution (with its bias) of the
    rounded operands, inside the bound of tests/test_gpu_sconv_edge64.py:test_fused_epilogues with bound(c) doubled:
        |y - y64| <= 2 bound(c) |invstd w| (1 + 6 u) + 6 u ((|c| + |mean|) |invstd w| + |b| + |residual|).
    Observed worst error / bound on MI355X: 0.025."""
    f = Os(name, Cin, Cout)
    xb, Wb = _bf(f.x), _bf(f.W)
    mean, invstd, w, b = (v.double() for v in f.bn)
    c64, cb = R.conv64(xb, Wb, f.b, f.nbr), 2 * R.bound(xb, Wb, f.b, f.nbr)
    scale = (invstd * w).abs()
    worst = 0.0
    for residual, relu in ((f.res, 1), (None, 1), (f.res, 0), (None, 0)):
        y64 = ((c64 - mean) * invstd) * w + b
        mag = (c64.abs() + mean.abs()) * scale + b.abs()
        if residual is not None:
            y64, mag = y64 + residual.double(), mag + residual.double().abs()
        if relu:
            y64 = y64.clamp(min=0)
        bnd = cb * scale * (1 + 6 * R.U) + 6 * R.U * mag
        what = f"{name} {Cin}->{Cout} residual {residual is not None} relu {relu}"
        worst = max(worst, _inside(f.os_bn(f.x, residual, relu), y64, bnd, what + " os_bn_bf16"),
                    _inside(f.two_pass_bn(f.x, residual, relu), y64, bnd, what + " gemm_bf16 + reduce_rows_bn"))
    record_property("worst_error_over_bound", worst)


# ------------------------------------------------------------------ poisoned rows
def _rows_hit(got, clean, hit, what):
    """rows in `hit` are non-finite in every element, every other row carries the bits of the clean run"""
    hit = torch.as_tensor(np.asarray(hit), device=got.device)
    assert bool((~torch.isfinite(got[hit])).all()), f"{what}: a row that meets a poisoned row came out finite"
    assert torch.equal(got[~hit], clean[~hit]), f"{what}: a row that meets no poisoned row changed"


@pytest.mark.parametrize("value", [NAN, float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("Cin,Cout", [(32, 32), (128, 96)], ids=["32x32", "128x96"])
@pytest.mark.parametrize("name", ["isolated", "line_x129"])
def test_poisoned_rows_reach_exactly_their_neighbours(name, Cin, Cout, value):
    """rows {0, a middle row, the last row} of x set to NaN / +Inf.  Both kernels load a missing neighbour (and the rows
    behind the end of a tile) from row 0 and mask it: that is right only while the mask is a select.  No ReLU here
    (max(NaN, 0) may legitimately be 0)."""
    f = Os(name, Cin, Cout)
    n, m = f.n, f.m
    rows = {0, n // 2, n - 1}
    xp = f.x.clone()
    xp[torch.as_tensor(sorted(rows), device="cuda")] = value
    hit = R.touched(f.nbr, rows)
    assert hit.any() and not hit.all()
    _, pin, _ = R.pairs(f.nbr)
    what = f"{name} {Cin}->{Cout} {value}"
    _rows_hit(f.product(xp), f.product(f.x), np.isin(pin, list(rows)), what + " product rows")
    for residual in (f.res, None):
        _rows_hit(f.os_bn(xp, residual, 0), f.os_bn(f.x, residual, 0), hit, what + " os_bn_bf16")
        _rows_hit(f.two_pass_bn(xp, residual, 0), f.two_pass_bn(f.x, residual, 0), hit, what + " gemm_bf16 + reduce_rows_bn")
    # the kinds without product rows: the scattered transposed k2 s2 and the identity
    for kind in ("tr_k2s2", "identity"):
        n_in, nbr = _nbr(name, kind)
        x, W, b = _operands(n_in, nbr.shape[0], Cin, Cout, 5)
        (Wp,) = _pack(W)
        bad = {0, n_in // 2, n_in - 1}
        xq = x.clone()
        xq[torch.as_tensor(sorted(bad), device="cuda")] = value
        _rows_hit(_conv_two_pass(kind, name, xq, Wp, b, Cin, Cout)[0], _conv_two_pass(kind, name, x, Wp, b, Cin, Cout)[0],
                  R.touched(nbr, bad), f"{what} {kind}")


# ------------------------------------------------------------------ models
# max |logits_bf16 - logits_fp32| / max |logits_fp32|, measured once on MI355X against the fp32 path (DESIGN.md section
# 3r); the bar is twice that.  The kernels are deterministic: the margin only covers a later change of accumulation order.
MEASURED = {
    ("MinkUNet34", 1): 0.0028654, ("MinkUNet34", 2): 0.00282231,
    ("MinkUNet34IBN", 1): 0.00565577, ("MinkUNet34IBN", 2): 0.00538501,
}


def _model(kind, seed=5):
    import lidog_amd
    from helpers import seeded_state_dict
    model = getattr(lidog_amd, kind)(in_channels=1, out_channels=7, D=3)
    model.load_state_dict(seeded_state_dict(model, seed=seed))
    return model.cuda().eval()


@pytest.mark.parametrize("os_mode", [1, 2], ids=["two_pass_convolutions", "output_stationary_convolutions"])
@pytest.mark.parametrize("kind", ["MinkUNet34", "MinkUNet34IBN"])
def test_model_routes_logits_and_no_state_leak(kind, os_mode, monkeypatch, record_property):
    import lidog_amd.me as ME
    from lidog_amd import precision, synth
    from lidog_amd.evaluate import predict
    monkeypatch.setattr(ME, "_SCONV_OS", os_mode)      # 2: every 3^3 same-stride map takes the output-stationary kernels
    monkeypatch.setattr(ME, "_OS_HINT", {})
    model = _model(kind)
    b = synth.make_batch([3, 4], "source8k", "cuda")
    C, feats = b["coords_int"], b["source_features0"]
    assert 4000 <= C.shape[0] <= 20000
    _, before = predict(model, C, feats)
    with precision.bf16_inference(model) as ctx:
        _, lg = predict(model, C, feats)
        _, inner_fp32 = predict(model, C, feats, precision="fp32")
    _, by_argument = predict(model, C, feats, precision="bf16")
    _, after = predict(model, C, feats)
    _, after_fp32 = predict(model, C, feats, precision="fp32")
    # (a) no state leaks: fp32 before, inside (suspended), and after a bf16 call: the same bits
    assert torch.equal(before, after) and torch.equal(before, inner_fp32) and torch.equal(before, after_fp32)
    assert precision.current() is None
    assert torch.equal(lg, by_argument), "the bf16 path is deterministic, however it is asked for"
    assert not torch.equal(lg, before), "the bf16 call ran the fp32 kernels"
    # (b) routes: every eligible convolution on a bf16 route, the stem and the classifier on fp32
    convs = {n: m for n, m in model.named_modules() if isinstance(m, ME._ConvBase)}
    assert ctx.kernels.packs == 1
    for n, m in convs.items():
        routes = ctx.routes.get(m, set())
        if precision.eligible(m):
            assert routes and routes <= set(precision.BF16_ROUTES), (n, routes)
        else:
            assert routes == {precision.FP32} and n in ("conv0p1s1", "final"), (n, routes)
    assert ctx.launches[precision.FP32] == 2 and sum(ctx.launches.values()) == len(convs), dict(ctx.launches)
    if os_mode == 2:
        assert ctx.launches[precision.OS_BN] > 0 and ctx.launches[precision.GEMM_REDUCE_BN] > 0    # 3^3 s1 / k2 s2
    else:
        assert ctx.launches[precision.OS_BN] == 0 and ctx.launches[precision.GEMM_REDUCE_BN] > 0
    assert ctx.launches[precision.GEMM_DIRECT] > 0                  # the 1x1 downsamples and the transposed k2 s2
    # (c) distance to the fp32 logits
    assert bool(torch.isfinite(lg).all())
    rel = float((lg - before).abs().max() / before.abs().max())
    print(f"{kind} os_mode {os_mode}: max |bf16 - fp32| / max |fp32| = {rel:.6g}, routes {dict(ctx.launches)}")
    record_property("relative_logit_distance", rel)
    assert rel <= 2.0 ** -5, f"{rel}: a finding to explain, not a bar to set"
    measured = MEASURED[kind, os_mode]
    assert measured is not None, f"no measured value recorded for this case (this run: {rel:.6g})"
    assert rel <= 2 * measured, f"{rel} against the measured {measured}"


# ------------------------------------------------------------------ end to end
def test_target_evaluator_bf16_packs_once(monkeypatch):
    from lidog_amd import evaluate, precision
    from lidog_amd.train import SynthScans
    packs = []
    refresh = precision.Bf16Kernels.refresh
    monkeypatch.setattr(precision.Bf16Kernels, "refresh", lambda self: (packs.append(1), refresh(self))[1])
    model = _model("MinkUNet34", seed=11)
    data = SynthScans(3, "source8k", first=10 ** 6)
    ev = evaluate.TargetEvaluator(model, precision="bf16")
    assert packs == [], "nothing is packed before a run"
    res = ev.run(evaluate.dataset_batches(data, 2), 3, rows="scan")            # two batches: 2 + 1 scans
    assert packs == [1] and ev.kernels.packs == 1
    assert res["scans"] == 3 and list(res["batch_of_scan"]) == [0, 0, 1]
    assert res["per_class"].shape == (7,) and np.isfinite(res["per_class"]).all() and np.isfinite(res["mean"])
    assert precision.current() is None
    # the fp32 evaluator over the same scans: the same voxels counted, an mIoU of its own
    ref = evaluate.TargetEvaluator(model).run(evaluate.dataset_batches(data, 2), 3, rows="scan")
    assert packs == [1]
    assert int(res["counts"].sum()) == int(ref["counts"].sum())
    print(f"mIoU bf16 {res['mean']:.4f} fp32 {ref['mean']:.4f}")


def test_fit_validates_in_bf16_with_one_pack_per_pass(monkeypatch):
    """Fit(val_precision="bf16"): a validation pass packs once, takes the bf16 routes, leaves no table current, and its
    loss is the fp32 pass's to within the logits' distance; the fp32 pass before and after gives the same numbers"""
    from lidog_amd import precision
    from lidog_amd.train import Fit, SynthScans
    packs = []
    refresh = precision.Bf16Kernels.refresh
    monkeypatch.setattr(precision.Bf16Kernels, "refresh", lambda self: (packs.append(1), refresh(self))[1])
    val = SynthScans(4, "source8k", first=10 ** 6)
    fit = Fit(model_kind="MinkUNet34", batch_size=2, epochs=0, train_data=SynthScans(2, "source8k"), val_data=val,
              num_sanity_val_steps=0, log=lambda *_: None, val_precision="bf16")
    half = fit.validate(0)
    assert packs == [1] and half["steps"] == 2 and precision.current() is None
    fit.val_precision = None
    full = fit.validate(0)
    fit.val_precision = "fp32"
    assert fit.validate(0) == full and packs == [1]
    assert half["sem_loss"] != full["sem_loss"], "the bf16 pass ran the fp32 kernels"
    assert abs(half["sem_loss"] - full["sem_loss"]) <= 2.0 ** -5 * abs(full["sem_loss"])
