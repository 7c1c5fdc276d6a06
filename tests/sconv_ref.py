"""Float64 yardstick of the sparse convolution's forward pass and data gradient, written from the definition and from
the coordinates alone: plain numpy / torch on the CPU, importing neither the package under test nor the CPU oracle (which
shares the rule book's conventions with the kernels).  tests/test_sconv_ref_cpu.py pins it to dense float64
F.conv3d / F.conv_transpose3d and their autograd on every scene below; tests/test_gpu_sconv_edge64.py holds the HIP
kernels of csrc/sconv.hip, csrc/sconv_mfma.hip, csrc/sconv_os.hip and the maps of csrc/coords.hip to it.

Conventions: coordinates are int32 [n, 4] rows (batch, x, y, z); the offsets of a kernel of size ks on
a map of tensor stride s_in are indexed x fastest, then y, then z; an odd ks is centred ((i - ks // 2) * s_in * dilation),
an even ks starts at 0 (i * s_in * dilation); a strided map holds floor(c / s) * s (toward -infinity) of every
coordinate, duplicates collapsed, rows in first-occurrence order.

The scenes are built for the edges a LiDAR-shaped scene never shows: offsets without pairs, offsets with 127 / 128 / 129
pairs (the gathered GEMM's tiles are 128 rows and never straddle an offset), rows with every neighbour or with the centre
only, two scans with the same coordinates, coordinates at the ends of the hash key's range."""
import numpy as np
import torch

U = 2.0 ** -24          # unit roundoff of float32
_BIAS = 1 << 20         # the yardstick's own key fields: wider than the +-65536 the library documents


# ------------------------------------------------------------------ neighbour sets
def offsets(ks, s_in, dilation=1):
    """[K, 3] (dx, dy, dz), index x fastest"""
    ks = int(ks)
    if ks % 2:
        r = [(i - ks // 2) * s_in * dilation for i in range(ks)]
    else:
        r = [i * s_in * dilation for i in range(ks)]
    return np.array([(x, y, z) for z in r for y in r for x in r], dtype=np.int64)


def _keys(c):
    """one Python integer per row (b, x, y, z): three 21-bit fields in an int64, the batch above them in Python's unbounded
    integers -- no two rows of any batch index and any coordinate within +-2^20 share a key"""
    c = np.asarray(c, dtype=np.int64)
    assert (np.abs(c[:, 1:]) < _BIAS).all() and (c[:, 0] >= 0).all()
    xyz = ((c[:, 1] + _BIAS) * (2 * _BIAS) + c[:, 2] + _BIAS) * (2 * _BIAS) + c[:, 3] + _BIAS        # < 2^63
    return [(b << 63) | k for b, k in zip(c[:, 0].tolist(), xyz.tolist())]


def strided(coords, s):
    """coordinates of the map of tensor stride s under `coords`: floor toward -infinity, first-occurrence order"""
    c = np.asarray(coords, dtype=np.int64).copy()
    c[:, 1:] = np.floor_divide(c[:, 1:], s) * s          # numpy floors (-7 // 2 == -4), C truncates
    seen, keep = set(), []
    for i, k in enumerate(_keys(c)):
        if k not in seen:
            seen.add(k)
            keep.append(i)
    return c[keep].astype(np.int32)


def neighbours(coords_in, coords_out, ks, s_in, s_out, dilation=1, offs=None):
    """nbr [K, n_out] int64: row of coords_in that holds coords_out[o] + offset k, or -1.  A dictionary from
    (b, x, y, z) -- as one integer key -- to row, probed per offset; a neighbour the library's range cannot hold is simply
    not in it.  `offs` replaces the offset list (the wrong variants of the CPU test)."""
    cin, cout = np.asarray(coords_in, dtype=np.int64), np.asarray(coords_out, dtype=np.int64)
    assert (cin[:, 1:] % s_in == 0).all() and (cout[:, 1:] % s_out == 0).all()
    table = {}
    for i, k in enumerate(_keys(cin)):
        assert k not in table, "duplicate input coordinate"
        table[k] = i
    offs = offsets(ks, s_in, dilation) if offs is None else np.asarray(offs, dtype=np.int64)
    nbr = np.empty((offs.shape[0], cout.shape[0]), dtype=np.int64)
    probe = cout.copy()
    for k, d in enumerate(offs):
        probe[:, 1:] = cout[:, 1:] + d
        nbr[k] = [table.get(q, -1) for q in _keys(probe)]
    return nbr


def transpose_map(nbr, n_in):
    """the exchanged map: nbr_t [K, n_in], nbr_t[k][i] = the output row o with nbr[k][o] == i, or -1 (for one offset
    o -> i is a shift, so there is at most one)"""
    nbr = np.asarray(nbr)
    out = np.full((nbr.shape[0], n_in), -1, dtype=np.int64)
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        assert np.unique(nbr[k][o]).size == o.size
        out[k, nbr[k][o]] = o
    return out


def pairs(nbr):
    """(k_off [K + 1], pair_in [P], pair_out [P]) of the rule book: per offset the pairs in ascending output row"""
    nbr = np.asarray(nbr)
    k_off, pin, pout = [0], [], []
    for k in range(nbr.shape[0]):
        o = np.nonzero(nbr[k] >= 0)[0]
        pin.append(nbr[k][o])
        pout.append(o)
        k_off.append(k_off[-1] + o.size)
    return (np.array(k_off, dtype=np.int64), np.concatenate(pin).astype(np.int64) if pin else np.zeros(0, np.int64),
            np.concatenate(pout).astype(np.int64) if pout else np.zeros(0, np.int64))


# ------------------------------------------------------------------ convolution in float64
def _gathered(x, nbr_k):
    """rows x[nbr_k] with zeros where nbr_k < 0 (a select: a non-finite row 0 must not leak)"""
    idx = torch.as_tensor(np.asarray(nbr_k), dtype=torch.long).to(x.device)
    g = x[idx.clamp(min=0)]
    return torch.where((idx >= 0).unsqueeze(1), g, torch.zeros((), dtype=x.dtype, device=x.device))


def conv64(x, W, b, nbr):
    """y[o] = sum_k x[nbr[k][o]] . W[k] (+ b): float32 (or float64) inputs, float64 accumulation, on the device of x.
    [n_out, Cout]"""
    x, W = x.detach().double(), W.detach().double()
    y = torch.zeros((np.asarray(nbr).shape[1], W.shape[2]), dtype=torch.float64, device=x.device)
    for k in range(W.shape[0]):
        y += _gathered(x, nbr[k]) @ W[k]
    if b is not None:
        y += b.detach().double().view(1, -1)
    return y


def dgrad64(gy, W, nbr, addend=None, n_in=None):
    """transpose of conv64 in x: gx[i] = sum_k sum_{o: nbr[k][o] == i} gy[o] . W[k]^T (+ addend).  [n_in, Cin]"""
    n_in = addend.shape[0] if n_in is None else n_in
    gx = conv64(gy, W.detach().transpose(1, 2), None, transpose_map(nbr, n_in))
    if addend is not None:
        gx += addend.detach().double()
    return gx


def tconv64(x, W, b, nbr, n_fine):
    """transposed convolution on the exchanged map: nbr [K, n_coarse] is the map fine -> coarse of the strided
    convolution; y[f] = sum over (k, c) with nbr[k][c] == f of x[c] . W[k] (+ b).  [n_fine, Cout]"""
    return conv64(x, W, b, transpose_map(nbr, n_fine))


def abs_terms(x, W, b, nbr, addend=None):
    """sum_k sum_ci |x||W| + |b| + |addend| per output element (float64)"""
    t = conv64(x.detach().abs(), W.detach().abs(), None if b is None else b.detach().abs(), nbr)
    if addend is not None:
        t += addend.detach().double().abs()
    return t


def bound(x, W, b, nbr, addend=None):
    """Forward error bound, per output element, of ANY float32 evaluation of conv64 that rounds at most Cin times per
    product row and adds the K product rows, the bias and the addend with at most K + 1 further additions, in any order:

        (Cin + K + 2) u (sum_k sum_ci |x||W| + |b| + |addend|) + K Cin 2^-126,      u = 2^-24.

    Derivation (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 and 3.4).  Every float32 operation returns
    the exact result times (1 + d), |d| <= u, unless it underflows.  A product row is a chain of Cin multiply-adds (fused
    or not: at most one rounding per term and partial sum that matters), so each term x W of it carries at most Cin
    factors (1 + d); the K + 1 additions that follow put at most K + 1 more on every term, bias and addend included.
    A computed element is therefore sum_t term_t (1 + theta_t) with |theta_t| <= (1 + u)^n - 1 =: gamma_n,
    n = Cin + K + 1, and its error is at most gamma_n sum_t |term_t|.  gamma_n = n u / (1 - n u) <= (n + 1) u as long as
    n (n + 1) u <= 1, which holds for n < 4095 (here n <= 384 + 125 + 1).  Underflow: a product or partial sum below
    2^-126 is rounded to a multiple of 2^-149 or flushed to zero, an absolute error below 2^-126 per multiply-add, of
    which an element has K Cin; additions of float32 numbers never lose anything to underflow.  Nothing here is measured
    on the kernels."""
    K, Cin = W.shape[0], W.shape[1]
    return (Cin + K + 2) * U * abs_terms(x, W, b, nbr, addend) + K * Cin * 2.0 ** -126


def worst_ratio(got, ref64, bnd):
    """max |got - ref| / bound (inf for a NaN or an infinity in `got`)"""
    got = got.detach().double().to(ref64.device)
    if not torch.isfinite(got).all():
        return float("inf")
    return float(((got - ref64).abs() / bnd).max()) if got.numel() else 0.0


# ------------------------------------------------------------------ poisoning
def touched(nbr, rows):
    """boolean [n_out]: output rows whose neighbour set meets `rows` (rows of the input matrix)"""
    nbr = np.asarray(nbr)
    return np.isin(nbr, np.asarray(list(rows), dtype=np.int64)).any(axis=0)


# ------------------------------------------------------------------ scenes
def _finish(c, seed):
    """shuffled rows (fixed seed), with a voxel that has the most 3^3 neighbours of its scene in row 0"""
    c = np.asarray(c, dtype=np.int64)
    c = c[np.random.default_rng(seed).permutation(c.shape[0])]
    count = (neighbours(c, c, 3, 1, 1) >= 0).sum(axis=0)
    best = int(np.argmax(count))
    c[[0, best]] = c[[best, 0]]
    return np.ascontiguousarray(c.astype(np.int32))


def _block(b, origin, size, keep=None):
    r = np.arange(size)
    x, y, z = np.meshgrid(r, r, r, indexing="ij")
    v = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    if keep is not None:
        v = v[keep(v)]
    v = v + np.asarray(origin)
    return np.concatenate([np.full((v.shape[0], 1), b), v], axis=1)


def _dense_cube():
    return _finish(np.concatenate([_block(0, (-4, 6, 0), 10), _block(1, (-4, 6, 0), 10)]), 1)


def _dense_cube_odd():
    return _finish(np.concatenate([_block(0, (-7, 5, -3), 10), _block(1, (-7, 5, -3), 10)]), 2)


def _isolated():
    x, y, z = np.meshgrid(np.arange(5), np.arange(7), np.arange(11), indexing="ij")
    v = 4 * np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1) + np.array([-8, 0, -20])
    return _finish(np.concatenate([np.zeros((v.shape[0], 1), np.int64), v], axis=1), 3)


def _line(axis, L):
    def build():
        v = np.zeros((L, 4), np.int64)
        v[:, 1:] = (3, -5, 2)
        v[:, axis] = np.arange(L) - 40
        return _finish(v, 4 + L + axis)
    return build


def _checkerboard():
    return _finish(_block(0, (-6, 0, 3), 12, keep=lambda v: v.sum(axis=1) % 2 == 0), 5)


def _small_scene(seed, n_points):
    from helpers import small_scene
    # a smaller extent than the default and no far points: the CPU test densifies the scene
    return small_scene(seed, n_points=n_points, extent=2.4, oob=0).astype(np.int64)


def _twin_scans():
    v = _small_scene(7, 2100)
    return _finish(np.concatenate([np.concatenate([np.full((v.shape[0], 1), b), v], axis=1) for b in (0, 1)]), 6)


def _one_and_many():
    v = _small_scene(8, 2600)
    many = np.concatenate([np.ones((v.shape[0], 1), np.int64), v], axis=1)
    one = many[v.shape[0] // 2:v.shape[0] // 2 + 1].copy()      # the same cell as a voxel of the other scan
    one[0, 0] = 0
    return _finish(np.concatenate([one, many]), 7)


def _tiny(n):
    return lambda: np.ascontiguousarray(_dense_cube()[:n])


def _range_ends():
    return _finish(np.concatenate([_block(0, (65533, 65533, 65533), 3), _block(4095, (-65536, -65536, -65536), 3)]), 8)


SCENES = {
    "dense_cube": _dense_cube,
    "dense_cube_odd": _dense_cube_odd,
    "isolated": _isolated,
    "line_x128": _line(1, 128),
    "line_x129": _line(1, 129),
    "line_x130": _line(1, 130),
    "line_z129": _line(3, 129),
    "checkerboard": _checkerboard,
    "twin_scans": _twin_scans,
    "one_and_many": _one_and_many,
    "tiny_1": _tiny(1),
    "tiny_2": _tiny(2),
    "tiny_127": _tiny(127),
    "tiny_128": _tiny(128),
    "tiny_129": _tiny(129),
    "range_ends": _range_ends,
}

# map kinds: name -> (kernel size, stride, dilation, transposed)
KINDS = {
    "k3s1": (3, 1, 1, False),
    "k5s1": (5, 1, 1, False),
    "k2s2": (2, 2, 1, False),
    "k3s2": (3, 2, 1, False),
    "k3s1d2": (3, 1, 2, False),
    "tr_k2s2": (2, 2, 1, True),
}
_CACHE = {}


def scene(name):
    if ("scene", name) not in _CACHE:
        _CACHE["scene", name] = SCENES[name]()
    return _CACHE["scene", name]


def scene_map(name, kind):
    """(coords_in, coords_out, nbr [K, n_out]) of a map kind on a scene, in the direction the convolution runs: for the
    transposed kind the input is the stride-2 map, the output the scene itself, and nbr the exchanged strided map.
    Cached: the tests share them and leave them unchanged."""
    key = ("map", name, kind)
    if key not in _CACHE:
        ks, stride, dil, transposed = KINDS[kind]
        fine = scene(name)
        coarse = strided(fine, stride) if stride > 1 else fine
        fwd = neighbours(fine, coarse, ks, 1, stride, dil)
        if transposed:
            _CACHE[key] = (coarse, fine, transpose_map(fwd, fine.shape[0]))
        else:
            _CACHE[key] = (fine, coarse, fwd)
    return _CACHE[key]
