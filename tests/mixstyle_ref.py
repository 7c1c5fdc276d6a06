"""Float64 yardstick of MixStyle (csrc/mixstyle.hip; the definition is the comment in include/lidog_amd.h), written from
the formulas in plain torch, and the bars the kernels are held to.  Everything runs in the dtype and on the device of its
inputs (float64 on the GPU for the GPU tests); tests/test_mixstyle_ref_cpu.py checks it against the paper's expressions
per scan (torch.var(unbiased=True), autograd with detached statistics) and shows that the bars pass a correct fp32
evaluation and fail five mutants.

Definitions (x [n, C], batch [n] the scan of every row, B scans, n_b rows in scan b; lam [B] fp32, partner [B], eps the
float32 1e-6 widened to double):
  mu[b, c] = sum x / n_b,  var[b, c] = max(0, (sum x^2 - (sum x)^2 / n_b) / (n_b - 1)) (unbiased),  sig = sqrt(var + eps),
  mu_mix = lam_b mu_b + (1 - lam_b) mu_p,  sig_mix = lam_b sig_b + (1 - lam_b) sig_p,  p = partner[b],
  sub = mu_b,  scale = sig_mix / sig_b,  add = mu_mix  (three fp32 tables, each rounded once from double),
  y = fmaf(x - sub[b], scale[b], add[b]),  dx = dy * scale[b]  (fp32).
A scan without rows has mu = 0, one with fewer than two rows var = 0.  An identity scan (n_b < 2, n_p < 2, p == b or
lam_b == 1) has the table row (0, 1, 0) exactly.
The float64 variance here is taken around the mean (sum (x - mu)^2 / (n_b - 1)): the same number, without the
cancellation of the sums form, so that the yardstick's own error stays at a few 2^-53.

Bars (each derived next to its function; `sums_bar`, `ulp32`, `U`, `U64` are those of tests/sparse_ref.py, the
propagation follows sparse_ref.stats_bounds with the unbiased divisor):
  mean, sub              1 fp32 ulp of the float64 value + gamma_{n_b} sum|x| / n_b
  sig                    1 ulp + d_var / sig, d_var what the double sums of n_b terms carry into the sums form
  add                    1 ulp + lam d_mu_b + (1 - lam) d_mu_p
  scale                  1 ulp + (d_sig_mix + scale d_sig_b) / (sig_b - d_sig_b)
  identity rows          exactly (0, 1, 0)
  y                      elementwise from the kernel's OWN fp32 tables, C_Y u (|x - sub| |scale| + |add|), C_Y = 2.02
  dx                     bit for bit: the fp32 product dy * scale[b] of the kernel's own scale
A non-finite value in a kernel output makes its ratio NaN, which fails every `<= 1` (outputs are pre-filled with NaN)."""
import math

import numpy as np
import torch

import inorm_ref as IR
import sparse_ref as R

U, U64 = R.U, R.U64
EPS = float(np.float32(1e-6))       # lidog_amd.me.MIXSTYLE_EPS as the C ABI receives it
# y = fmaf(x - sub, scale, add): the subtraction rounds once (u |x - sub|, carried through the product: u |x - sub| |scale|),
# the fused multiply-add rounds once (u |y| <= u (|x - sub| |scale| + |add|)): at most 2 u (|x - sub| |scale| + |add|),
# 1 % for second order
C_Y = 2.02


# ------------------------------------------------------------------ float64 definitions
def moments64(x, batch, B, eps=EPS):
    """per (b, c): cnt [B], mu, unbiased var (around the mean), sig, and the sums s1 = sum x, s2 = sum x^2,
    s1_abs = sum |x| that the bars start from"""
    i = batch.long()
    s1, s2, s1_abs = IR._per_scan(x, batch, B), IR._per_scan(x * x, batch, B), IR._per_scan(x.abs(), batch, B)
    cnt = torch.bincount(i, minlength=B)
    nb = cnt.to(x.dtype)[:, None]
    mu = s1 / nb.clamp_min(1)
    dev2 = IR._per_scan((x - mu[i]) ** 2, batch, B)
    var = torch.where(nb > 1, dev2 / (nb - 1).clamp_min(1), torch.zeros_like(dev2))
    return dict(cnt=cnt, mu=mu, var=var, sig=torch.sqrt(var + eps), s1=s1, s2=s2, s1_abs=s1_abs)


def identity_scans(cnt, lam, partner):
    """bool [B]: n_b < 2, n_p < 2, partner[b] == b or lam_b == 1"""
    p = partner.long()
    b = torch.arange(cnt.numel(), device=cnt.device)
    return (cnt < 2) | (cnt[p] < 2) | (p == b) | (lam.float() == 1.0)


def tables64(m, lam, partner):
    """(sub, scale, add, ident) [B, C] float64 from moments64's dict; identity scans hold (0, 1, 0)"""
    p = partner.long()
    ident = identity_scans(m["cnt"], lam, partner)
    l = lam.to(m["mu"].dtype)[:, None]
    mu_mix = l * m["mu"] + (1.0 - l) * m["mu"][p]
    sig_mix = l * m["sig"] + (1.0 - l) * m["sig"][p]
    idc = ident[:, None]
    sub = torch.where(idc, torch.zeros_like(mu_mix), m["mu"])
    scale = torch.where(idc, torch.ones_like(mu_mix), sig_mix / m["sig"])
    add = torch.where(idc, torch.zeros_like(mu_mix), mu_mix)
    return sub, scale, add, ident


def mixstyle_y64(x, batch, sub, scale, add):
    """y = (x - sub[b]) scale[b] + add[b] and the magnitude scale |x - sub| |scale| + |add| of its fp32 evaluation"""
    i = batch.long()
    core = (x - sub[i]) * scale[i]
    return core + add[i], core.abs() + add[i].abs()


def mixstyle64(x, batch, B, lam, partner, eps=EPS):
    """y of the definition in one call (float64 x)"""
    sub, scale, add, _ = tables64(moments64(x, batch, B, eps), lam, partner)
    return mixstyle_y64(x, batch, sub, scale, add)[0]


# ------------------------------------------------------------------ bars
def moment_bounds(m, eps=EPS):
    """(d_mu, d_sig) [B, C]: what double sums of n_b terms (each within gamma_{n_b} sum|terms|, sparse_ref.sums_bar)
    carry into mu = s1 / n and sig = sqrt((s2 - s1^2 / n) / (n - 1) + eps):
      |d s1| <= gamma_n s1_abs, |d s2| <= gamma_n s2,
      |d (s2 - s1^2 / n)| <= |d s2| + (2 |s1| |d s1| + |d s1|^2) / n + 4 2^-53 s2   (the roundings of the expression),
      |d var| = that / (n - 1);  |sqrt(a + d) - sqrt(a)| <= |d| / sqrt(a), so |d sig| <= |d var| / sig + 4 2^-53 sig.
    Scans with fewer than two rows have var = 0 by definition (d_sig = 0); a scan without rows has d_mu = 0 too."""
    d_mu, d_sig = torch.zeros_like(m["mu"]), torch.zeros_like(m["mu"])
    for b, n in enumerate(m["cnt"].tolist()):
        if n == 0:
            continue
        d_s1, d_s2 = R.sums_bar(n, m["s1_abs"][b]), R.sums_bar(n, m["s2"][b])
        d_mu[b] = d_s1 / n + 2 * U64 * m["mu"][b].abs()
        if n > 1:
            d_var = (d_s2 + (2.0 * m["s1"][b].abs() * d_s1 + d_s1 * d_s1) / n + 4 * U64 * m["s2"][b]) / (n - 1)
            d_sig[b] = d_var / m["sig"][b] + 4 * U64 * m["sig"][b]
    return d_mu, d_sig


def table_ratios(o, x, batch, B, lam, partner, eps=EPS):
    """{'mean', 'sig', 'sub', 'scale', 'add', 'identity'}: the kernel's fp32 mean / sig / sub / scale / add [B, C]
    against float64.  With d_mu / d_sig of moment_bounds and l = lam_b:
      mean, sig    ulp32(ref) + d
      sub          as mean (bar 0 on identity rows: exactly 0)
      add          ulp32(ref) + l d_mu_b + (1 - l) d_mu_p + 4 2^-53 (|l mu_b| + |(1 - l) mu_p|)
      scale        sig_mix within d_sm = l d_sig_b + (1 - l) d_sig_p + 4 2^-53 sig_mix of its value; the quotient of two
                   perturbed numbers: |d scale| <= (d_sm + scale d_sig_b) / (sig_b - d_sig_b) + 4 2^-53 scale;
                   bar = ulp32(ref) + that
      identity     0 if every identity row is exactly (0, 1, 0), else inf"""
    C = x.shape[1]
    m = moments64(x.double(), batch, B, eps)
    d_mu, d_sig = moment_bounds(m, eps)
    sub, scale, add, ident = tables64(m, lam, partner)
    p = partner.long()
    l = lam.double()[:, None]
    idc = ident[:, None].expand(B, C)
    zero = torch.zeros_like(d_mu)
    d_add = l * d_mu + (1.0 - l) * d_mu[p] + 4 * U64 * ((l * m["mu"]).abs() + ((1.0 - l) * m["mu"][p]).abs())
    sig_mix = l * m["sig"] + (1.0 - l) * m["sig"][p]
    d_sm = l * d_sig + (1.0 - l) * d_sig[p] + 4 * U64 * sig_mix
    d_scale = (d_sm + scale * d_sig) / (m["sig"] - d_sig).clamp_min(1e-300) + 4 * U64 * scale
    got = {k: o[k].reshape(B, C) for k in ("mean", "sig", "sub", "scale", "add")}
    r = {"mean": IR.ratio(got["mean"], m["mu"], R.ulp32(m["mu"]) + d_mu),
         "sig": IR.ratio(got["sig"], m["sig"], R.ulp32(m["sig"]) + d_sig),
         "sub": IR.ratio(got["sub"], sub, torch.where(idc, zero, R.ulp32(sub) + d_mu)),
         "scale": IR.ratio(got["scale"], scale, torch.where(idc, zero, R.ulp32(scale) + d_scale)),
         "add": IR.ratio(got["add"], add, torch.where(idc, zero, R.ulp32(add) + d_add))}
    exact = bool((got["sub"][ident] == 0).all() and (got["scale"][ident] == 1).all() and (got["add"][ident] == 0).all())
    r["identity"] = 0.0 if exact else math.inf
    return r


def elem_ratios(o, x, dy, batch, B, ident):
    """{'y', 'dx', 'identity_rows'}: y against float64 from the kernel's own fp32 tables within
    C_Y u (|x - sub| |scale| + |add|); dx equal to the fp32 product dy * scale[b] bit for bit (0 or inf); on the rows
    of identity scans y == x and dx == dy bit for bit (0 or inf)"""
    C = x.shape[1]
    sub, scale, add = (o[k].reshape(B, C) for k in ("sub", "scale", "add"))
    i = batch.long()
    ref, mag = mixstyle_y64(x.double(), batch, sub.double(), scale.double(), add.double())
    r = {"y": IR.elem_ratio(o["y"], ref, mag, C_Y)}
    r["dx"] = 0.0 if torch.equal(o["dx"], dy * scale[i]) else math.inf
    rows = ident[i]
    same = torch.equal(o["y"][rows], x[rows]) and torch.equal(o["dx"][rows], dy[rows])
    r["identity_rows"] = 0.0 if same else math.inf
    return r


def check(o, d, lam, partner, what):
    """o: mean, sig, sub, scale, add [B C], y, dx [n, C] of lidog_mixstyle_stats / _apply / _bwd on case d (an
    inorm_ref.make_case) with lam / partner [B] on d's device.  Returns the worst ratio per bar (all asserted <= 1)."""
    x, batch, B = d["x"], d["batch"], d["B"]
    r = table_ratios(o, x, batch, B, lam, partner)
    ident = identity_scans(torch.bincount(batch.long(), minlength=B), lam, partner)
    r.update(elem_ratios(o, x, d["dy"], batch, B, ident))
    IR.assert_ratios(r, what)
    return r


# ------------------------------------------------------------------ the draws the GPU tests use per layout
LAM_VALUES = (0.0, 1.0, 0.5, float(np.float32(np.random.RandomState(7).beta(0.1, 0.1))))


def combos(B):
    """[(name, lam float32 [B], partner int32 [B])]: a rotation by one, a map with fixed points (the even scans), and a
    non-permutation (every scan but the first shares partner 0); lam cycles through 0, 1, 0.5 and a Beta(0.1, 0.1) draw,
    starting one further in every combination"""
    b = np.arange(B)
    maps = [("rotation", (b + 1) % max(B, 1)),
            ("fixed_points", np.where(b % 2 == 0, b, (b + 1) % max(B, 1))),
            ("shared_partner", np.where(b == 0, min(1, B - 1), 0))]
    out = []
    for k, (name, partner) in enumerate(maps):
        lam = np.array([LAM_VALUES[(j + k + 2) % 4] for j in range(B)], dtype=np.float32)
        out.append((name, torch.from_numpy(lam), torch.from_numpy(partner.astype(np.int32))))
    return out


# ------------------------------------------------------------------ a correct fp32 evaluation (and its mutants) on the CPU
def evaluate32(x, dy, batch, B, lam, partner, eps=EPS, biased=False, swap_lam=False, inverse_partner=False):
    """What the kernels compute, in torch on the CPU: double sums per scan, the moments and the mix in double, the
    five tables rounded once to fp32, y = the fp32 difference times scale plus add rounded once (the product of two
    fp32 numbers is exact in double), dx the fp32 product.  The keyword arguments build the mutants of
    tests/test_mixstyle_ref_cpu.py."""
    C = x.shape[1]
    i = batch.long()
    xd = x.double()
    s1, s2 = IR._per_scan(xd, batch, B), IR._per_scan(xd * xd, batch, B)
    cnt = torch.bincount(i, minlength=B)
    nb = cnt.double()[:, None]
    mu = s1 / nb.clamp_min(1)
    div = nb if biased else nb - 1
    var = torch.where(nb > 1, torch.clamp_min((s2 - s1 * s1 / nb.clamp_min(1)) / div.clamp_min(1), 0.0),
                      torch.zeros_like(s1))
    sig = torch.sqrt(var + eps)
    p = partner.long()
    if inverse_partner:
        p = torch.argsort(p)
    l = lam.double()[:, None]
    if swap_lam:
        l = 1.0 - l
    ident = identity_scans(cnt, lam, partner)[:, None]
    one, zero = torch.ones_like(mu), torch.zeros_like(mu)
    sub = torch.where(ident, zero, mu).float()
    scale = torch.where(ident, one, (l * sig + (1.0 - l) * sig[p]) / sig).float()
    add = torch.where(ident, zero, l * mu + (1.0 - l) * mu[p]).float()
    diff = x - sub[i]
    y = (diff.double() * scale[i].double() + add[i].double()).float()
    return dict(mean=mu.float().reshape(-1), sig=sig.float().reshape(-1), sub=sub.reshape(-1), scale=scale.reshape(-1),
                add=add.reshape(-1), y=y, dx=dy * scale[i])
