"""Instance norm and the fused IBN pass (csrc/inorm.hip: lidog_in_segments, lidog_in_stats, lidog_in_apply,
lidog_in_bwd_reduce, lidog_in_bwd_apply, lidog_ibn_apply, lidog_ibn_bwd_reduce, lidog_ibn_bwd_apply) through the C ABI
against the float64 yardstick and the derived bars of tests/inorm_ref.py, on the layouts of inorm_ref.LAYOUTS: scans of
1 .. 4 RB + 1 rows, empty scans (leading, middle, trailing), 16 scans shorter than a row block inside one workgroup,
scan boundaries next to workgroup boundaries, either side of the 256-workgroup cap, per_wg no multiple of RB, every
float4 width and the scalar kernels, both sides of the 2 B C = 4096 gate, the second radix pass of the segments
(B > 512); then MinkowskiInstanceNorm and ibn_relu through autograd (fused and the literal fallback).

Every output (mean, invstd, coef, dw, db, y, dx, perm, seg_off, bid, bits, and the workspaces) is pre-filled with NaN /
an impossible integer; ReLU decisions come from the kernel's own bits, which are asserted equal to y > 0; no element is
left out of a comparison.

Worst ratio to each bar observed on an MI355X (gfx950) over all layouts and the module tests (every case records its own
with record_property): mean, invstd, m0, m1, dw, db 0.50 (the fp32 cast: half an ulp of a bar of one ulp); y 0.69;
dx 0.46; IBN: y (BatchNorm half) 0.71, bn sum g 0.00, bn sum g xhat 0.12, bn dw / db 0.50, in m0 / m1 / dw / db 0.50,
fused dx 0.51."""
import pytest
import torch

import inorm_ref as IR

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _fill(shape, value, dtype):
    """the integer outputs and the byte workspace, pre-filled with an impossible value"""
    return torch.full(shape, value, dtype=dtype, device="cuda")


def _dev(t):
    """every float operand the tests own"""
    return t.cuda()


def _case(lay):
    """inorm_ref.make_case on the GPU with its float tensors through _dev"""
    d = IR.make_case(lay, "cuda")
    return {k: _dev(v) if torch.is_tensor(v) and v.is_floating_point() else v for k, v in d.items()}


def _segments(batch, B):
    """lidog_in_segments on coords [n, 4] whose batch column is `batch`; outputs pre-filled with -7"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    n = batch.numel()
    coords = torch.zeros((max(n, 1), 4), dtype=torch.int32, device="cuda")
    coords[:n, 0] = batch
    coords[:n, 1] = torch.arange(n, device="cuda", dtype=torch.int32)
    perm, bid = (_fill((max(n, 1),), -7, torch.int32) for _ in range(2))
    seg_off = _fill((B + 1,), -7, torch.int32)
    nbytes = L.lidog_in_segments_ws(n)
    ws = _fill((nbytes,), 0xA5, torch.uint8)
    call("lidog_in_segments", ptr(coords), n, B, ptr(perm), ptr(seg_off), ptr(bid), ptr(ws), nbytes)
    torch.cuda.synchronize()
    return perm[:n], seg_off, bid[:n]


def _check_segments(perm, seg_off, bid, batch, B):
    rperm, rseg, _ = IR.segments64(batch, B)
    assert torch.equal(perm.long(), rperm), "perm is not the stable batch order"
    assert torch.equal(seg_off.long(), rseg), "seg_off"
    assert torch.equal(bid, batch), "bid"


def _run_in(d, segs):
    """the four stand-alone entries; every output and the workspace pre-filled with NaN"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    perm, seg_off, bid = segs
    n, C, B, x, dy = d["n"], d["C"], d["B"], d["x"], d["dy"]
    o = dict(mean=_nan(B * C), invstd=_nan(B * C), y=_nan(n, C), coef=_nan(2 * B * C), dw=_nan(C), db=_nan(C),
             dx=_nan(n, C))
    ws = _nan(L.lidog_in_reduce_ws(B, C), dtype=torch.float64)
    call("lidog_in_stats", ptr(x), n, C, B, ptr(perm), ptr(seg_off), 1e-8, ptr(o["mean"]), ptr(o["invstd"]), ptr(ws))
    call("lidog_in_apply", ptr(x), n, C, B, ptr(bid), ptr(o["mean"]), ptr(o["invstd"]), ptr(d["w"]), ptr(d["b"]),
         ptr(o["y"]))
    ws2 = _nan(L.lidog_in_reduce_ws(B, C), dtype=torch.float64)
    call("lidog_in_bwd_reduce", ptr(dy), ptr(x), n, C, B, ptr(perm), ptr(seg_off), ptr(o["mean"]), ptr(o["invstd"]),
         ptr(ws2), ptr(o["coef"]), ptr(o["dw"]), ptr(o["db"]))
    call("lidog_in_bwd_apply", ptr(dy), ptr(x), n, C, B, ptr(bid), ptr(o["mean"]), ptr(o["invstd"]), ptr(d["w"]),
         ptr(o["coef"]), ptr(o["dx"]))
    torch.cuda.synchronize()
    return o


def _run_ibn(d, segs, o):
    """lidog_bn_stats + the three fused entries on the instance-norm statistics `o` of _run_in"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    perm, seg_off, bid = segs
    n, C, B, x, dy2 = d["n"], d["C"], d["B"], d["x"], d["dy2"]
    q = dict(bn_mean=_nan(C), bn_invstd=_nan(C), in_mean=o["mean"], in_invstd=o["invstd"], y_in=o["y"],
             y=_nan(n, 2 * C), bits=_fill((L.lidog_relu_bits_words(n, 2 * C),), -1, torch.int32),
             bn_sums=_nan(2 * C + 1, dtype=torch.float64), bn_dw=_nan(C), bn_db=_nan(C), coef=_nan(2 * B * C),
             in_dw=_nan(C), in_db=_nan(C), dx=_nan(n, C))
    fsums = _nan(2 * C + 1, dtype=torch.float64)
    bn_ws = _nan(max(L.lidog_bn_reduce_ws(C, 1), 1), dtype=torch.float64)
    call("lidog_bn_stats", ptr(x), n, C, 1, ptr(fsums), ptr(bn_ws), float(n), 1e-5, 0.0, ptr(q["bn_mean"]),
         ptr(q["bn_invstd"]), None, None)
    call("lidog_ibn_apply", ptr(x), n, C, B, ptr(q["bn_mean"]), ptr(q["bn_invstd"]), ptr(d["bn_w"]), ptr(d["bn_b"]),
         ptr(bid), ptr(o["mean"]), ptr(o["invstd"]), ptr(d["w"]), ptr(d["b"]), ptr(q["y"]), ptr(q["bits"]))
    bn_ws2 = _nan(max(L.lidog_bn_reduce_ws(C, 1), 1), dtype=torch.float64)
    in_ws = _nan(L.lidog_in_reduce_ws(B, C), dtype=torch.float64)
    call("lidog_ibn_bwd_reduce", ptr(dy2), ptr(q["bits"]), ptr(x), n, C, B, ptr(q["bn_mean"]), ptr(q["bn_invstd"]),
         ptr(q["bn_sums"]), ptr(bn_ws2), ptr(q["bn_dw"]), ptr(q["bn_db"]), ptr(perm), ptr(seg_off), ptr(o["mean"]),
         ptr(o["invstd"]), ptr(in_ws), ptr(q["coef"]), ptr(q["in_dw"]), ptr(q["in_db"]))
    call("lidog_ibn_bwd_apply", ptr(dy2), ptr(q["bits"]), ptr(x), n, C, B, ptr(q["bn_mean"]), ptr(q["bn_invstd"]),
         ptr(d["bn_w"]), ptr(q["bn_sums"]), float(n), ptr(bid), ptr(o["mean"]), ptr(o["invstd"]), ptr(d["w"]),
         ptr(q["coef"]), ptr(q["dx"]))
    torch.cuda.synchronize()
    return q


def _record(record_property, r, prefix=""):
    for k, v in r.items():
        record_property(prefix + k, v)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("lay", IR.LAYOUTS, ids=[lay["id"] for lay in IR.LAYOUTS])
def test_instance_norm_and_ibn_entries_vs_float64(lay, record_property):
    d = _case(lay)
    segs = _segments(d["batch"], d["B"])
    _check_segments(*segs, d["batch"], d["B"])
    o = _run_in(d, segs)
    _record(record_property, IR.check_in(o, d, lay["id"]))
    if IR.vector_path(d["C"], d["B"]):
        q = _run_ibn(d, segs, o)
        _record(record_property, IR.check_ibn(q, d, lay["id"] + " ibn"), "ibn_")


@pytest.mark.timeout(60)
@pytest.mark.parametrize("B,n", [(512, 5000), (513, 5000), (4096, 5000), (4096, 0), (3, 0)])
def test_segments_radix_passes_and_empty_map(B, n):
    """one radix pass up to B = 512, two above; sparse batch ids (most scans empty); n = 0 writes seg_off = 0 only"""
    g = torch.Generator().manual_seed(B + n)
    batch = (torch.randint(0, B, (n,), generator=g) // 3 * 3).clamp_max(B - 1).to(torch.int32).cuda()
    if n:
        batch[n // 2] = B - 1                               # the largest id is present
    perm, seg_off, bid = _segments(batch, B)
    _check_segments(perm, seg_off, bid, batch, B)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("lid", ["n40k_C96_shuffled", "gate17_C128_shuffled"])
def test_three_runs_give_identical_bits(lid):
    """one layout of the float4 path (256 workgroups, the two-level tail) and one of the scalar path"""
    lay = next(la for la in IR.LAYOUTS if la["id"] == lid)
    d = IR.make_case(lay, "cuda")
    segs = _segments(d["batch"], d["B"])
    runs = []
    for _ in range(3):
        o = _run_in(d, segs)
        if IR.vector_path(d["C"], d["B"]):
            o.update({"ibn_" + k: v for k, v in _run_ibn(d, segs, o).items()})
        runs.append(o)
    for other in runs[1:]:
        for k, v in runs[0].items():
            assert torch.equal(v, other[k]), f"{lid}: {k} differs between runs"


# ------------------------------------------------------------------ the modules through autograd
MODULE_LAYOUTS = [dict(id="tiny16", C=32, sizes=IR.TINY, order="shuffled"),
                  dict(id="b17_literal", C=128, sizes=IR._uneven(4000, 17), order="shuffled"),
                  dict(id="empty_middle", C=64, sizes=[3000, 0, 2003], order="shuffled")]


def _sparse(ME, d, f):
    n = d["n"]
    i = torch.arange(n, dtype=torch.int32, device="cuda")
    coords = torch.stack([d["batch"], i % 64, (i // 64) % 64, i // 4096], dim=1).contiguous()
    st = ME.SparseTensor(f, coordinates=coords)
    assert torch.equal(st.C[:, 0], d["batch"]) and st.F.shape == f.shape
    return st


@pytest.mark.timeout(60)
@pytest.mark.parametrize("lay", MODULE_LAYOUTS, ids=[la["id"] for la in MODULE_LAYOUTS])
def test_modules_through_autograd_vs_float64(lay, record_property):
    """ME.MinkowskiInstanceNorm and ME.ibn_relu (fused where the shape allows, the literal composition at B = 17, C = 128)
    forward + backward; the statistics the bars start from are those the same kernels give through the C ABI on the
    coordinate manager's own segments (the kernels are bit-reproducible)"""
    import lidog_amd.me as ME
    from lidog_amd._lib import call, ptr
    d = IR.make_case(lay, "cuda")
    n, C, B = d["n"], d["C"], d["B"]
    f = d["x"].clone().requires_grad_(True)
    st = _sparse(ME, d, f)
    perm, seg_off, bid, mB = st.coordinate_manager.segments(st.coordinate_map_key)
    assert mB == B
    _check_segments(perm, seg_off, bid, d["batch"], B)
    own = _run_in(d, (perm, seg_off, bid))
    inn, bn = ME.MinkowskiInstanceNorm(C).cuda(), ME.MinkowskiBatchNorm(C).cuda()
    with torch.no_grad():
        inn.weight.copy_(d["w"][None])
        inn.bias.copy_(d["b"][None])
        bn.bn.weight.copy_(d["bn_w"])
        bn.bn.bias.copy_(d["bn_b"])
    y = inn(st).F
    y.backward(d["dy"])
    o = dict(mean=own["mean"], invstd=own["invstd"], coef=own["coef"], y=y.detach(), dx=f.grad.clone(),
             dw=inn.weight.grad.clone(), db=inn.bias.grad.clone())
    _record(record_property, IR.check_in(o, d, lay["id"] + " module"))
    for k in ("y", "dx", "dw", "db"):
        assert torch.equal(o[k].reshape(-1), own[k].reshape(-1)), f"module {k} differs from the C ABI's"
    # ibn_relu
    f.grad = inn.weight.grad = inn.bias.grad = None
    out = ME.ibn_relu(bn, inn, st).F
    fused = type(out.grad_fn).__name__ == "_IBNReluFnBackward"
    assert fused == IR.vector_path(C, B), "ibn_relu took the other path"
    out.backward(d["dy2"])
    q = dict(bn_mean=torch.full((C,), NAN, device="cuda"), bn_invstd=torch.full((C,), NAN, device="cuda"),
             in_mean=own["mean"], in_invstd=own["invstd"], y_in=own["y"], y=out.detach(), bits=IR.pack_bits(out.detach() > 0),
             bn_dw=bn.bn.weight.grad.clone(), bn_db=bn.bn.bias.grad.clone(), in_dw=inn.weight.grad.clone(),
             in_db=inn.bias.grad.clone(), dx=f.grad.clone(), coef=_nan(2 * B * C))
    from lidog_amd import _lib
    L = _lib.load()
    sums = _nan(2 * C + 1, dtype=torch.float64)
    ws = _nan(max(L.lidog_bn_reduce_ws(C, 1), 1), dtype=torch.float64)
    call("lidog_bn_stats", ptr(d["x"]), n, C, 1, ptr(sums), ptr(ws), float(n), 1e-5, 0.0, ptr(q["bn_mean"]),
         ptr(q["bn_invstd"]), None, None)
    g_in = torch.where(out.detach()[:, C:] > 0, d["dy2"][:, C:], torch.zeros_like(d["dy2"][:, C:])).contiguous()
    ws2 = _nan(L.lidog_in_reduce_ws(B, C), dtype=torch.float64)
    dw_, db_ = _nan(C), _nan(C)
    call("lidog_in_bwd_reduce", ptr(g_in), ptr(d["x"]), n, C, B, ptr(perm), ptr(seg_off), ptr(own["mean"]),
         ptr(own["invstd"]), ptr(ws2), ptr(q["coef"]), ptr(dw_), ptr(db_))
    torch.cuda.synchronize()
    _record(record_property, IR.check_ibn(q, d, lay["id"] + " ibn_relu"), "ibn_")
