"""tests/inorm_ref.py checked without a GPU: its float64 definitions against F.instance_norm + autograd on every scan's
rows; segments64 against numpy's stable argsort; and its bars against a plain-torch fp32 evaluation of the kernels'
formulas (double sums, fp32 elementwise expressions in the kernels' operation order): every bar passes on every layout
of the GPU test, and the statistics bars fail once a scan boundary is moved by one row or one row of a 3-row scan is
left out of the sums."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inorm_ref as IR
import sparse_ref as R

BY_ID = {lay["id"]: lay for lay in IR.LAYOUTS}


# ------------------------------------------------------------------ the definitions against F.instance_norm
@pytest.mark.parametrize("lid", ["tiny16_C32_shuffled", "3000x0x2003_C32_shuffled", "one11_C96_shuffled",
                                 "width_C7_shuffled", "gate17_C128_shuffled"])
def test_float64_definitions_equal_instance_norm_autograd_per_scan(lid):
    """y, dx, dweight, dbias of inorm_ref in float64 against F.instance_norm on [1, C, n_b] of every scan and its
    autograd.  Tolerance 1e-12 of the largest sum of term magnitudes per channel (dx of a two-row scan is a difference
    of equal terms: |ref| itself is no scale), plus 64 * 2^-53 times the condition
    E[x^2] / (var + eps) of the variance-from-sums formula the yardstick (like the kernels) uses -- 1e6 on the channel
    of mean 1e3, which F.instance_norm's centred variance does not pay.  F.instance_norm refuses a scan of one row:
    there y = bias and dx = 0 by the definition (x = mean, g = m0)."""
    d = IR.make_case(BY_ID[lid])
    B, C, batch = d["B"], d["C"], d["batch"]
    x, g, w, b = (d[k].double() for k in ("x", "dy", "w", "b"))
    s = IR.in_stats64(x, batch, B)
    i = batch.long()
    xhat = (x - s["mean"][i]) * s["invstd"][i]
    bs = IR.in_bwd_sums64(g, xhat, batch, B)
    nb = s["cnt"].double().clamp_min(1)[:, None]
    y, y_scale = IR.in_y64(x, batch, s["mean"], s["invstd"], w, b)
    dx, dx_scale = IR.in_dx64(g, x, batch, s["mean"], s["invstd"], w, bs["sg"] / nb, bs["sgx"] / nb)
    dw_ref, db_ref = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    cond = (s["s2"] / nb) / (s["var"] + IR.EPS)
    for sc in range(B):
        rows = (batch == sc).nonzero().flatten()
        if rows.numel() == 0:
            assert torch.equal(s["mean"][sc], torch.zeros(C, dtype=torch.float64))
            assert torch.equal(s["invstd"][sc], torch.full((C,), 1.0 / np.sqrt(IR.EPS), dtype=torch.float64))
            continue
        if rows.numel() == 1:
            assert torch.equal(y[rows[0]], b) and torch.equal(dx[rows[0]], torch.zeros(C, dtype=torch.float64))
            db_ref += g[rows[0]]
            continue
        xs = x[rows].t()[None].clone().requires_grad_(True)
        ws, bs_ = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        ys = F.instance_norm(xs, weight=ws, bias=bs_, use_input_stats=True, eps=IR.EPS)
        ys.backward(g[rows].t()[None])
        tol = 1e-12 + 64 * R.U64 * cond[sc]
        for got, ref, scale, what in ((y[rows], ys.detach()[0].t(), y_scale[rows], "y"),
                                      (dx[rows], xs.grad[0].t(), dx_scale[rows], "dx")):
            err = (got - ref).abs().amax(0)
            assert bool((err <= tol * scale.amax(0).clamp_min(1e-30)).all()), (what, sc, float((err / tol).max()))
        dw_ref += ws.grad
        db_ref += bs_.grad
    scale_w = bs["a_dw"] * (1e-12 + 64 * R.U64 * cond.amax(0)) + 1e-30
    assert bool(((bs["dw"] - dw_ref).abs() <= scale_w).all()), "dweight"
    assert bool(((bs["db"] - db_ref).abs() <= 1e-12 * bs["a_db"] + 1e-30).all()), "dbias"


@pytest.mark.parametrize("B,n", [(3, 5003), (513, 5000), (4096, 5000), (4, 0)])
def test_segments64_is_numpy_stable_argsort(B, n):
    g = torch.Generator().manual_seed(B + n)
    batch = (torch.randint(0, B, (n,), generator=g) // 3 * 3).clamp_max(B - 1).to(torch.int32)   # sparse ids
    perm, seg_off, counts = IR.segments64(batch, B)
    c = batch.numpy()
    assert np.array_equal(perm.numpy(), np.argsort(c, kind="stable"))
    assert np.array_equal(counts.numpy(), np.bincount(c, minlength=B))
    assert np.array_equal(seg_off.numpy(), np.concatenate([[0], np.cumsum(np.bincount(c, minlength=B))]))


# ------------------------------------------------------------------ the kernels' formulas in plain torch fp32
def _stats32(x, kbatch, cnt, keep):
    """fp32 mean / invstd [B, C] from double sums over the rows `keep` keyed by kbatch, divided by cnt"""
    B = cnt.numel()
    xd = x.double()[keep]
    kb = kbatch[keep]
    s1, s2 = IR._per_scan(xd, kb, B), IR._per_scan(xd * xd, kb, B)
    n = cnt.double()[:, None]
    m = torch.where(n > 0, s1 / n.clamp_min(1), torch.zeros_like(s1))
    var = torch.where(n > 0, torch.clamp_min(s2 / n.clamp_min(1) - m * m, 0.0), torch.zeros_like(s1))
    return m.float(), (1.0 / torch.sqrt(var + IR.EPS)).float()


def _bwd32(g, x, kbatch, cnt, keep, mean, invstd):
    """fp32 coef [2, B, C], dw, db from double sums of g and g * xhat32"""
    B = cnt.numel()
    i = kbatch.long()
    xh = (x - mean[i]) * invstd[i]
    gd, gx = g.double()[keep], (g.double() * xh.double())[keep]
    sg, sgx = IR._per_scan(gd, kbatch[keep], B), IR._per_scan(gx, kbatch[keep], B)
    n = cnt.double()[:, None]
    z = torch.zeros_like(sg)
    coef = torch.stack([torch.where(n > 0, sg / n.clamp_min(1), z), torch.where(n > 0, sgx / n.clamp_min(1), z)]).float()
    return coef, sgx.sum(0).float(), sg.sum(0).float()


def _dx32(g, x, mu, is_, w, m0, m1):
    return (g - m0 - (x - mu) * is_ * m1) * (is_ * w)


def emulate(d, kbatch=None, cnt=None, keep=None, ibn=True):
    """what the kernels compute, in torch: `kbatch` / `cnt` / `keep` default to the truth; a test passes others to
    stand for a kernel that assigns a row to the wrong scan or leaves one out of its sums"""
    x, B, C, n = d["x"], d["B"], d["C"], d["n"]
    kbatch = d["batch"] if kbatch is None else kbatch
    cnt = torch.bincount(d["batch"].long(), minlength=B) if cnt is None else cnt
    keep = torch.ones(n, dtype=torch.bool) if keep is None else keep
    i = kbatch.long()
    mean, invstd = _stats32(x, kbatch, cnt, keep)
    o = dict(mean=mean.reshape(-1), invstd=invstd.reshape(-1))
    o["y"] = (x - mean[i]) * invstd[i] * d["w"] + d["b"]
    coef, o["dw"], o["db"] = _bwd32(d["dy"], x, kbatch, cnt, keep, mean, invstd)
    o["coef"] = coef.reshape(-1)
    o["dx"] = _dx32(d["dy"], x, mean[i], invstd[i], d["w"], coef[0][i], coef[1][i])
    if not (ibn and IR.vector_path(C, B)):
        return o, None
    xd = x.double()
    s1, s2 = xd.sum(0), (xd * xd).sum(0)
    bm = s1 / n
    q = dict(bn_mean=bm.float(), bn_invstd=(1.0 / torch.sqrt(torch.clamp_min(s2 / n - bm * bm, 0.0) + IR.BN_EPS)).float(),
             in_mean=o["mean"], in_invstd=o["invstd"], y_in=o["y"])
    y_bn = (x - q["bn_mean"]) * q["bn_invstd"] * d["bn_w"] + d["bn_b"]
    q["y"] = torch.relu(torch.cat([y_bn, o["y"]], dim=1))
    q["bits"] = IR.pack_bits(q["y"] > 0)
    g = torch.where(q["y"] > 0, d["dy2"], torch.zeros_like(d["dy2"]))
    g_bn, g_in = g[:, :C].contiguous(), g[:, C:].contiguous()
    xh = (x - q["bn_mean"]) * q["bn_invstd"]
    sg, sgx = g_bn.double().sum(0), (g_bn.double() * xh.double()).sum(0)
    q["bn_sums"] = torch.cat([sg, sgx, torch.tensor([float(n)], dtype=torch.float64)])
    q["bn_db"], q["bn_dw"] = sg.float(), sgx.float()
    coef, q["in_dw"], q["in_db"] = _bwd32(g_in, x, kbatch, cnt, keep, mean, invstd)
    q["coef"] = coef.reshape(-1)
    q["dx"] = _dx32(g_bn, x, q["bn_mean"], q["bn_invstd"], d["bn_w"], (sg / n).float(), (sgx / n).float()) + \
        _dx32(g_in, x, mean[i], invstd[i], d["w"], coef[0][i], coef[1][i])
    return o, q


@pytest.mark.parametrize("lay", IR.LAYOUTS, ids=[lay["id"] for lay in IR.LAYOUTS])
def test_every_bar_passes_a_correct_fp32_evaluation(lay):
    d = IR.make_case(lay)
    o, q = emulate(d)
    IR.check_in(o, d, lay["id"])
    if q is not None:
        IR.check_ibn(q, d, lay["id"] + " ibn")


def _stat_bars(o, d):
    B, C = d["B"], d["C"]
    i = d["batch"].long()
    r = IR.stats_ratios(o["mean"], o["invstd"], d["x"], d["batch"], B)
    mean, invstd = o["mean"].reshape(B, C), o["invstd"].reshape(B, C)
    r.update(IR.bwd_ratios(o["coef"], o["dw"], o["db"], d["dy"], (d["x"] - mean[i]) * invstd[i], d["batch"], B))
    return r


@pytest.mark.parametrize("lid", ["3000x0x2003_C32_shuffled", "tiny16_C32_collated", "wgedge_C64_shuffled"])
def test_statistics_bars_fail_a_scan_boundary_moved_by_one_row(lid):
    """the last sorted row of the first scan counted to the next scan that has rows (seg_off moved by one): mean,
    invstd, m0, m1 and dweight leave their bars; dbias, the sum of g over ALL rows, cannot see it"""
    d = IR.make_case(BY_ID[lid])
    assert max(_stat_bars(emulate(d, ibn=False)[0], d).values()) <= 1.0
    perm, seg_off, counts = IR.segments64(d["batch"], d["B"])
    src = 0
    dst = next(b for b in range(1, d["B"]) if d["sizes"][b])
    if d["sizes"][src] < 2:                       # keep the first scan non-empty: take the first scan with >= 2 rows
        src = next(b for b in range(d["B"]) if d["sizes"][b] >= 2)
        dst = next(b for b in range(src + 1, d["B"]) if d["sizes"][b])
    row = perm[seg_off[src + 1] - 1]
    kbatch, cnt = d["batch"].clone(), counts.clone()
    kbatch[row] = dst
    cnt[src] -= 1
    cnt[dst] += 1
    r = _stat_bars(emulate(d, kbatch=kbatch, cnt=cnt, ibn=False)[0], d)
    assert all(r[k] > 1.0 for k in ("mean", "invstd", "m0", "m1", "dw")), r


def test_statistics_bars_fail_a_row_dropped_from_a_three_row_scan():
    """one row of a 3-row scan left out of every sum (the count stays 3): every statistics bar fails, dbias too"""
    d = IR.make_case(BY_ID["tiny16_C32_shuffled"])
    sc = d["sizes"].index(3)
    keep = torch.ones(d["n"], dtype=torch.bool)
    keep[(d["batch"] == sc).nonzero().flatten()[1]] = False
    r = _stat_bars(emulate(d, keep=keep, ibn=False)[0], d)
    assert all(v > 1.0 for v in r.values()), r


def test_bars_fail_stale_and_unwritten_outputs():
    """a NaN left in any output, a wrong placeholder of an empty scan, and one wrong ReLU bit are all seen"""
    d = IR.make_case(BY_ID["3000x0x2003_C32_shuffled"])
    o, q = emulate(d)
    C = d["C"]
    for key, idx in (("mean", C + 3), ("invstd", C + 3), ("coef", C + 3), ("coef", 4 * C + 3)):
        bad = dict(o)
        bad[key] = o[key].clone()
        bad[key][idx] = bad[key][idx] + 1e-3        # slot of the empty scan 1
        with pytest.raises(AssertionError):
            IR.check_in(bad, d, key)
    for key in ("mean", "invstd", "coef", "dw", "db", "y", "dx"):
        bad = dict(o)
        bad[key] = o[key].clone()
        bad[key].view(-1)[-1] = float("nan")
        with pytest.raises(AssertionError):
            IR.check_in(bad, d, key)
    for key in ("y", "bn_sums", "bn_dw", "bn_db", "coef", "in_dw", "in_db", "dx"):
        bad = dict(q)
        bad[key] = q[key].clone()
        bad[key].view(-1)[1] = float("nan")
        with pytest.raises(AssertionError):
            IR.check_ibn(bad, d, key)
    bad = dict(q)
    bad["bits"] = q["bits"].clone()
    bad["bits"][5] ^= 4
    with pytest.raises(AssertionError):
        IR.check_ibn(bad, d, "bits")
