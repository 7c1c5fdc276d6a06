"""MixStyle (csrc/mixstyle.hip: lidog_mixstyle_stats, lidog_mixstyle_apply, lidog_mixstyle_bwd) through the C ABI
against the float64 yardstick and the derived bars of tests/mixstyle_ref.py, on the layouts of inorm_ref.LAYOUTS (scans
of 1 .. 4 RB + 1 rows, empty scans, 16 tiny scans in one workgroup, scan boundaries at workgroup edges, both sides of the
256-workgroup cap, every float4 width and the scalar kernels, both sides of the 2 B C = 4096 gate), each with three
partner maps (a rotation by one, a map with fixed points, a non-permutation) and lam holding 0, 1, 0.5 and a
Beta(0.1, 0.1) draw; then MinkowskiMixStyle through autograd.

Every output and the workspace are pre-filled with NaN; no element is left out of a comparison; dx is compared bit for
bit with the fp32 product of the kernel's own scale; identity scans must hold (0, 1, 0) and leave their rows alone.

Worst ratio to each bar observed on an MI355X (gfx950) over all layouts, combinations and the module tests (every case
records its own with record_property): mean, sig, sub, scale, add 0.50 (the fp32 cast: half an ulp of a bar of one ulp);
y 0.96 (1.93 u against the bar's 2.02 u); dx, identity tables and identity rows 0 (exact)."""
import numpy as np
import pytest
import torch

import inorm_ref as IR
import mixstyle_ref as MR

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, dtype=dtype, device="cuda")


def _segments(batch, B):
    """lidog_in_segments on coords [n, 4] whose batch column is `batch`"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    n = batch.numel()
    coords = torch.zeros((max(n, 1), 4), dtype=torch.int32, device="cuda")
    coords[:n, 0] = batch
    coords[:n, 1] = torch.arange(n, device="cuda", dtype=torch.int32)
    perm, bid = (torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    seg_off = torch.full((B + 1,), -7, dtype=torch.int32, device="cuda")
    nbytes = L.lidog_in_segments_ws(n)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    call("lidog_in_segments", ptr(coords), n, B, ptr(perm), ptr(seg_off), ptr(bid), ptr(ws), nbytes)
    torch.cuda.synchronize()
    return perm[:n], seg_off, bid[:n]


def _run(d, segs, lam, partner):
    """the three entries; lam / partner are host tensors; every output and the workspace pre-filled with NaN"""
    from lidog_amd import _lib
    from lidog_amd._lib import call, ptr
    L = _lib.load()
    perm, seg_off, bid = segs
    n, C, B, x, dy = d["n"], d["C"], d["B"], d["x"], d["dy"]
    o = {k: _nan(B * C) for k in ("mean", "sig", "sub", "scale", "add")}
    o.update(y=_nan(n, C), dx=_nan(n, C))
    ws = _nan(L.lidog_mixstyle_ws(B, C), dtype=torch.float64)
    call("lidog_mixstyle_stats", ptr(x), n, C, B, ptr(perm), ptr(seg_off), ptr(lam), ptr(partner), MR.EPS,
         ptr(o["mean"]), ptr(o["sig"]), ptr(o["sub"]), ptr(o["scale"]), ptr(o["add"]), ptr(ws))
    call("lidog_mixstyle_apply", ptr(x), n, C, B, ptr(bid), ptr(o["sub"]), ptr(o["scale"]), ptr(o["add"]), ptr(o["y"]))
    call("lidog_mixstyle_bwd", ptr(dy), n, C, B, ptr(bid), ptr(o["scale"]), ptr(o["dx"]))
    torch.cuda.synchronize()
    return o


def _record(record_property, r, prefix=""):
    for k, v in r.items():
        record_property(prefix + k, v)


@pytest.mark.timeout(60)
@pytest.mark.parametrize("lay", IR.LAYOUTS, ids=[lay["id"] for lay in IR.LAYOUTS])
def test_mixstyle_entries_vs_float64(lay, record_property):
    d = IR.make_case(lay, "cuda")
    segs = _segments(d["batch"], d["B"])
    worst = {}
    for name, lam, partner in MR.combos(d["B"]):
        o = _run(d, segs, lam, partner)
        r = MR.check(o, d, lam.cuda(), partner.cuda(), f"{lay['id']} {name}")
        for k, v in r.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if d["C"] >= 2:       # the channel that is constant within a scan: var = 0 exactly, sig = sqrt(eps), scale = 1
            sig, scale = o["sig"].reshape(d["B"], -1), o["scale"].reshape(d["B"], -1)
            assert torch.equal(sig[:, 1], torch.full_like(sig[:, 1], float(np.float32(np.sqrt(np.float64(MR.EPS))))))
            assert torch.equal(scale[:, 1], torch.ones_like(scale[:, 1]))
    _record(record_property, worst)


@pytest.mark.timeout(60)
def test_out_of_range_partner_is_an_error_before_any_launch():
    from lidog_amd import _lib
    lay = next(la for la in IR.LAYOUTS if la["id"] == "wgedge_C64_shuffled")
    d = IR.make_case(lay, "cuda")
    segs = _segments(d["batch"], d["B"])
    lam = torch.full((d["B"],), 0.5)
    for bad in (-1, d["B"]):
        partner = torch.zeros(d["B"], dtype=torch.int32)
        partner[d["B"] - 1] = bad
        with pytest.raises(RuntimeError, match="partner"):
            _run(d, segs, lam, partner)
        assert b"partner" in _lib.load().lidog_last_error()
    # nothing was queued: the outputs of a refused call keep their fill
    from lidog_amd._lib import ptr, stream
    L = _lib.load()
    B, C, n = d["B"], d["C"], d["n"]
    o = {k: _nan(B * C) for k in ("mean", "sig", "sub", "scale", "add")}
    ws = _nan(L.lidog_mixstyle_ws(B, C), dtype=torch.float64)
    partner = torch.full((B,), B, dtype=torch.int32)
    rc = L.lidog_mixstyle_stats(ptr(d["x"]), n, C, B, ptr(segs[0]), ptr(segs[1]), ptr(lam), ptr(partner), MR.EPS,
                                ptr(o["mean"]), ptr(o["sig"]), ptr(o["sub"]), ptr(o["scale"]), ptr(o["add"]), ptr(ws),
                                stream())
    torch.cuda.synchronize()
    assert rc != 0
    for v in list(o.values()) + [ws]:
        assert bool(torch.isnan(v).all())


@pytest.mark.timeout(60)
@pytest.mark.parametrize("lid", ["n40k_C96_shuffled", "gate17_C128_shuffled"])
def test_two_calls_give_identical_bytes(lid):
    """one layout of the float4 path (256 workgroups, the two-level tail) and one of the scalar path"""
    lay = next(la for la in IR.LAYOUTS if la["id"] == lid)
    d = IR.make_case(lay, "cuda")
    segs = _segments(d["batch"], d["B"])
    _, lam, partner = MR.combos(d["B"])[0]
    a, b = _run(d, segs, lam, partner), _run(d, segs, lam, partner)
    for k, v in a.items():
        assert torch.equal(v.view(torch.int32), b[k].view(torch.int32)), f"{lid}: {k} differs between calls"


# ------------------------------------------------------------------ the module through autograd
MODULE_LAYOUTS = [dict(id="tiny16", C=32, sizes=IR.TINY, order="shuffled"),
                  dict(id="b17_scalar", C=128, sizes=IR._uneven(4000, 17), order="shuffled"),
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
def test_module_through_autograd_vs_float64(lay, record_property):
    """MinkowskiMixStyle forward + backward with the draws given, and with the module's own draws (p = 1): values and
    gradient against the float64 restatement through the bars; the tables the bars start from are those the same
    kernels give through the C ABI on the coordinate manager's own segments (the kernels are bit-reproducible)"""
    import lidog_amd.me as ME
    from lidog_amd.data import draw_mixstyle
    d = IR.make_case(lay, "cuda")
    B = d["B"]
    f = d["x"].clone().requires_grad_(True)
    st = _sparse(ME, d, f)
    perm, seg_off, bid, mB = st.coordinate_manager.segments(st.coordinate_map_key)
    assert mB == B
    mod = ME.MinkowskiMixStyle(p=1.0, alpha=0.1, seed=[3, 1]).cuda()
    assert not list(mod.parameters()) and not list(mod.buffers()) and mod.eps == ME.MIXSTYLE_EPS
    twin = np.random.RandomState([3, 1])
    for k, (name, lam, partner) in enumerate(MR.combos(B)[:2] + [("own",) + tuple(
            torch.from_numpy(a) for a in draw_mixstyle(twin, B, 1.0, 0.1))]):
        f.grad = None
        out = mod(st) if name == "own" else mod(st, draws=(lam.numpy(), partner.numpy()))
        assert out is not st and out.coordinate_map_key == st.coordinate_map_key
        out.F.backward(d["dy"])
        own = _run(d, (perm, seg_off, bid), lam, partner)
        o = dict(own, y=out.F.detach(), dx=f.grad.clone())
        _record(record_property, MR.check(o, d, lam.cuda(), partner.cuda(), f"{lay['id']} module {name}"), name + "_")
        for key in ("y", "dx"):
            assert torch.equal(o[key], own[key]), f"module {key} differs from the C ABI's"


@pytest.mark.timeout(60)
def test_module_is_the_identity_in_eval_mode_and_when_the_gate_fails():
    import lidog_amd.me as ME
    d = IR.make_case(MODULE_LAYOUTS[2], "cuda")
    st = _sparse(ME, d, d["x"].clone())
    mod = ME.MinkowskiMixStyle(p=1.0).cuda()
    state = mod.rng.get_state()[1].copy()
    assert mod.eval()(st) is st
    assert np.array_equal(mod.rng.get_state()[1], state)          # eval mode draws nothing
    assert mod.train()(st) is not st
    assert ME.MinkowskiMixStyle(p=0.0).cuda().train()(st) is st
    with pytest.raises(ValueError):
        mod(st, draws=(np.zeros(d["B"] + 1, np.float32), np.zeros(d["B"] + 1, np.int32)))
    with pytest.raises(RuntimeError, match="partner"):
        mod(st, draws=(np.zeros(d["B"], np.float32), np.full(d["B"], d["B"], np.int32)))
