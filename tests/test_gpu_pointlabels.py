"""The point-level kernels on the GPU (csrc/pointlabels.hip behind lidog_amd.scans.keep_rows and
lidog_amd.evaluate.point_labels) against their numpy restatement (tests/pointlabels_ref.py), exactly: the keep index at
every size where the two-level scan takes another path, on rows at, one ulp inside and around the radius, the labels and
the confusion for 2 to 20 classes over batches with empty and wholly dropped scans, a (label, prediction) pair past
2^16 points, every bit of the error word, and the agreement with the voxel-level predictions at every voxel's first
point."""
import numpy as np
import pytest
import torch

import pointlabels_ref as P
from lidog_amd import evaluate, scans

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1024, 1025, 3 * 1024 + 7)
PATTERNS = ("all", "none", "alternating", "last")
RADIUS = 50.0


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _records(n, stride, pattern, seed):
    """[n, stride] float32 records whose radius mask follows `pattern`; the columns past z hold large values the mask
    must not read"""
    rng = np.random.default_rng([seed, n, stride])
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    keep = {"all": np.ones(n, bool), "none": np.zeros(n, bool), "alternating": np.arange(n) % 2 == 0,
            "last": np.arange(n) == n - 1}[pattern]
    r = np.where(keep, rng.uniform(0.5, 49.0, n), rng.uniform(51.0, 90.0, n))
    rec = np.full((n, stride), 1.0e6, dtype=np.float32)
    rec[:, :3] = (d * r[:, None]).astype(np.float32)
    assert np.array_equal(P.radius_mask_np(rec[:, :3], RADIUS), keep)
    return rec, keep


def _check_keep(rec, stride, in_radius=RADIUS):
    want, m = P.keep_rows_np(rec, stride, in_radius)
    dev = _cuda(rec.reshape(-1))
    keep_row, count = scans.keep_rows(dev, stride, in_radius)
    assert keep_row.dtype == torch.int32 and keep_row.shape == (rec.shape[0],) and count.shape == (1,)
    got = keep_row.cpu().numpy()
    assert np.array_equal(got, want) and int(count) == m
    # the records with an index are load_scan's points, bit for bit and in its order
    loaded = scans.load_scan(dev, None, None, stride, in_radius=in_radius)["points"].cpu().numpy()
    assert np.array_equal(rec[got >= 0, :3].view(np.uint32), loaded.view(np.uint32))
    return got


# ------------------------------------------------------------------ keep index
@pytest.mark.parametrize("stride", [3, 4, 5])
def test_keep_rows_sizes_and_patterns(stride):
    for n in SIZES:
        for pattern in PATTERNS:
            rec, keep = _records(n, stride, pattern, 1)
            got = _check_keep(rec, stride)
            assert np.array_equal(got >= 0, keep), (n, pattern)
    # raw bytes are taken as the same words; without a radius every record keeps its own number
    rec, _ = _records(1025, stride, "alternating", 2)
    k, m = scans.keep_rows(_cuda(rec.reshape(-1).view(np.uint8)), stride, RADIUS)
    assert np.array_equal(k.cpu().numpy(), P.keep_rows_np(rec, stride, RADIUS)[0]) and int(m) == 513
    k, m = scans.keep_rows(_cuda(rec.reshape(-1)), stride, None)
    assert np.array_equal(k.cpu().numpy(), np.arange(1025)) and int(m) == 1025
    with pytest.raises(ValueError, match="multiple"):
        scans.keep_rows(_cuda(rec.reshape(-1)[:-1]), stride, RADIUS)


def _fma_sum(p):
    """x x + y y + z z with the products fused into the sums: fma(z, z, fma(y, y, x x)), each step rounded to float32
    once (the products of two float32 are exact in float64)"""
    x, y, z = (p[:, i].astype(np.float64) for i in range(3))
    t = (x * x).astype(np.float32)
    t = (y * y + t.astype(np.float64)).astype(np.float32)
    return (z * z + t.astype(np.float64)).astype(np.float32)


@pytest.mark.parametrize("stride", [3, 4, 5])
def test_keep_rows_at_the_radius(stride):
    rng = np.random.default_rng(7)
    d = rng.normal(size=(20000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = (d * (RADIUS * (1.0 + rng.uniform(-3e-7, 3e-7, 20000)))[:, None]).astype(np.float32)
    plain = P.radius_mask_np(shell, RADIUS)
    fused = _fma_sum(shell) < np.float32(RADIUS) ** 2
    differ = np.nonzero(plain != fused)[0]
    assert differ.size > 0 and plain.any() and not plain.all()         # the case is not vacuous
    inside = np.nextafter(np.float32(RADIUS), np.float32(0))
    special = np.array([[RADIUS, 0, 0], [inside, 0, 0], [0, -RADIUS, 0], [0, 0, inside], [30, 40, 0],
                        [np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan], [np.inf, 0, 0], [0, -np.inf, 0], [1, 2, 3]],
                       dtype=np.float32)
    pts = np.concatenate([special, shell[differ], shell[:3000]])
    rec = np.full((pts.shape[0], stride), np.nan, dtype=np.float32)    # a NaN past z is not a coordinate
    rec[:, :3] = pts
    got = _check_keep(rec, stride)
    assert (got[:11] >= 0).tolist() == [False, True, False, True, False, False, False, False, False, False, True]
    assert np.array_equal(got[11:11 + differ.size] >= 0, plain[differ])           # numpy's answer, not the fused one


# ------------------------------------------------------------------ point labels and confusion
def _logits(n, c, seed):
    """random float32 logits: a third of the rows on a grid of 0.5 (exact ties, often of the maximum), some rows with
    one or two NaN at any position"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, c), generator=g)
    grid = torch.randint(0, 3, (n, c), generator=g).float() * 0.5
    tied = torch.rand(n, generator=g) < 0.33
    x[tied] = grid[tied]
    nan_rows = torch.nonzero(torch.rand(n, generator=g) < 0.05).view(-1)
    x[nan_rows, torch.randint(0, c, (nan_rows.shape[0],), generator=g)] = float("nan")
    x[nan_rows[::2], torch.randint(0, c, (nan_rows[::2].shape[0],), generator=g)] = float("nan")
    if n > 4:
        x[1] = 0.25                                        # every class ties: class 0
        x[2] = float("nan")                                # every entry NaN: class 0
        x[3, :] = 0.0
        x[3, c - 1] = float("nan")                         # the NaN wins over the zeros
    return x.numpy()


LAYOUTS = {
    "one": [(2500, 0.9)],                                  # more than two blocks of 1024 rows
    "empty_middle": [(1500, 0.8), (0, 0.0), (700, 0.5)],   # a block holds rows of two scans around an empty one
    "all_dropped": [(300, 0.7), (200, 0.0), (900, 1.0)],   # a scan without kept rows and voxels
}


def _batch(layout, c, seed, kind="int32"):
    """a batch as point_labels takes it, on the host.  Every scan with kept rows has a voxel holding one point (0), a
    voxel holding 300 or as many as there are (1), a voxel holding none (2)"""
    rng = np.random.default_rng([seed, c])
    L = 40
    lut = rng.integers(-1, c, L).astype(np.int32)          # about 1 / (c + 1) of the raw ids are ignored
    lut[:c] = np.arange(c)
    lut[c] = -1
    keep_row, inverse, raw, row_off, kept_off, vox_off = [], [], [], [0], [0], [0]
    for n, p in LAYOUTS[layout]:
        keep = rng.random(n) < p
        m = int(keep.sum())
        keep_row.append(np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32))
        nv = 0
        if m:
            nv = max(4, m // 3)
            inv = rng.integers(3, nv, m)
            inv[0] = 0
            inv[1:1 + min(300, m - 1)] = 1
            inv = inv[rng.permutation(m)]
            assert (inv == 0).sum() == 1 and (inv == 1).sum() == min(300, m - 1) and not (inv == 2).any()
            inverse.append(inv.astype(np.int64))
        ids = rng.integers(0, L, n)
        raw.append((ids | (rng.integers(1, 1 << 15, n) << 16)).astype(np.int32) if kind == "int32" else ids.astype(np.uint8))
        row_off.append(row_off[-1] + n)
        kept_off.append(kept_off[-1] + m)
        vox_off.append(vox_off[-1] + nv)
    return dict(logits=_logits(vox_off[-1], c, seed), row_off=row_off, kept_off=kept_off, vox_off=vox_off,
                keep_row=np.concatenate(keep_row), inverse_map=np.concatenate(inverse + [np.zeros(0, np.int64)]),
                labels_raw=np.concatenate(raw), lut=lut, mask=0xFFFF if kind == "int32" else None)


def _run(b, out_lut=None, fill=0, labels=True, ignore_label=-1, err=None, counts=None, inverse_dtype=torch.int64):
    return evaluate.point_labels(
        _cuda(b["logits"]), b["row_off"], b["kept_off"], b["vox_off"], _cuda(b["keep_row"]),
        _cuda(b["inverse_map"]).to(inverse_dtype), None if out_lut is None else _cuda(np.asarray(out_lut, np.int32)), fill,
        _cuda(b["labels_raw"]) if labels else None, _cuda(b["lut"]) if labels else None, b["mask"], ignore_label, counts, err)


def _want(b, out_lut=None, fill=0, labels=True, ignore_label=-1):
    return P.point_labels_np(b["logits"], b["row_off"], b["kept_off"], b["vox_off"], b["keep_row"], b["inverse_map"],
                             out_lut, fill, b["labels_raw"] if labels else None, b["lut"], b["mask"], ignore_label)


@pytest.mark.parametrize("kind", ["int32", "uint8"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("c", [2, 7, 19, 20])
def test_point_labels_and_confusion(c, layout, kind):
    b = _batch(layout, c, 3, kind)
    n, nb = b["keep_row"].shape[0], len(b["row_off"]) - 1
    out_lut = (np.arange(c)[::-1] * 3 + 10).astype(np.int32)                # not the identity
    want, want_counts, err = _want(b, out_lut, 255)
    assert err == 0
    out, counts = _run(b, out_lut, 255)
    assert out.dtype == torch.uint32 and out.shape == (n,) and counts.dtype == torch.int64 and counts.shape == (nb, c, c)
    got = out.cpu().numpy()
    assert np.array_equal(got, want)                                         # every record
    assert (got[b["keep_row"] < 0] == 255).all() and (got[b["keep_row"] >= 0] != 255).all()
    assert np.array_equal(counts.cpu().numpy(), want_counts)
    mapped, _ = P.map_labels_np(b["labels_raw"], b["lut"], b["mask"])
    counted = (b["keep_row"] >= 0) & (mapped != -1)
    assert int(counts.sum()) == int(counted.sum()) and 0 < counted.sum() < (b["keep_row"] >= 0).sum()
    # the arg-max is the voxel-level evaluator's, ties and NaN rows included
    v = b["logits"].shape[0]
    preds, _ = evaluate.confusion(_cuda(b["logits"]), torch.zeros(v, dtype=torch.int64, device="cuda"),
                                  torch.zeros((v, 4), dtype=torch.int32, device="cuda"), 1)
    assert np.array_equal(preds.cpu().numpy(), P.argmax_np(b["logits"]))
    plain, _ = _run(b, labels=False)                                         # the identity, fill 0, no labels
    for s in range(nb):
        rows = np.arange(b["row_off"][s], b["row_off"][s + 1])
        rows = rows[b["keep_row"][rows] >= 0]
        vox = b["vox_off"][s] + b["inverse_map"][b["kept_off"][s] + b["keep_row"][rows]]
        assert np.array_equal(plain.cpu().numpy()[rows], preds.cpu().numpy()[vox])
    # two runs give the same bytes; counts are added to, also into a slice of a larger tensor; int32 inverse maps
    out2, counts2 = _run(b, out_lut, 255, inverse_dtype=torch.int32)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)) and torch.equal(counts, counts2)
    big = torch.zeros((nb + 3, c, c), dtype=torch.int64, device="cuda")
    _, acc = _run(b, out_lut, 255, counts=big[2:2 + nb])
    _run(b, out_lut, 255, counts=big[2:2 + nb])
    assert np.array_equal(big[2:2 + nb].cpu().numpy(), 2 * want_counts) and int(big[:2].sum() + big[2 + nb:].sum()) == 0
    # an in-range ignore label
    _, ci = _run(b, out_lut, 255, ignore_label=1)
    assert np.array_equal(ci.cpu().numpy(), _want(b, out_lut, 255, ignore_label=1)[1]) and int(ci[:, 1].sum()) == 0


def test_one_pair_past_65536_points():
    """70 000 kept records of one scan, one voxel, one label: a (label, prediction) bin a 16-bit counter could not hold"""
    n, c = 70000, 7
    logits = np.zeros((2, c), np.float32)
    logits[0, 4] = 1.0
    b = dict(logits=logits, row_off=[0, n], kept_off=[0, n], vox_off=[0, 2], keep_row=np.arange(n, dtype=np.int32),
             inverse_map=np.zeros(n, np.int64), labels_raw=np.full(n, 3, np.uint8),
             lut=np.array([-1, 0, 1, 2, 3], np.int32), mask=None)
    out, counts = _run(b)
    assert (out.cpu().numpy() == 4).all()
    want = np.zeros((1, c, c), np.int64)
    want[0, 2, 4] = n
    assert np.array_equal(counts.cpu().numpy(), want) and np.array_equal(_want(b)[1], want)


def test_error_word():
    clean = _batch("empty_middle", 7, 5)
    fill = 99
    ok_out, ok_counts, _ = _want(clean, None, fill)
    L = clean["lut"].shape[0]
    kept2 = np.nonzero(clean["keep_row"][1500:] >= 0)[0] + 1500              # kept records of the last scan
    cases = {}
    b = dict(clean, labels_raw=clean["labels_raw"].copy())
    b["labels_raw"][kept2[3]] = (5 << 16) | (L + 2)                          # a raw id past the table
    cases[P.ERR_LABEL] = (b, kept2[3])
    b = dict(clean, inverse_map=clean["inverse_map"].copy())
    rec = int(np.nonzero(clean["keep_row"][:1500] >= 0)[0][17])              # a kept record of scan 0
    b["inverse_map"][clean["kept_off"][0] + clean["keep_row"][rec]] = clean["vox_off"][1]     # the voxel row past scan 0's
    cases[P.ERR_INVERSE] = (b, rec)
    b = dict(clean, keep_row=clean["keep_row"].copy())
    b["keep_row"][kept2[10]] = clean["kept_off"][3] - clean["kept_off"][2]   # the first kept row past the last scan's
    cases[P.ERR_KEEP] = (b, kept2[10])
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    for bit, (b, rec) in cases.items():
        want, want_counts, e = _want(b, None, fill)
        assert e == bit and want[rec] == fill and np.array_equal(np.delete(want, rec), np.delete(ok_out, rec))
        assert want_counts.sum() in (ok_counts.sum() - 1, ok_counts.sum())   # an ignored record was never counted
        err = torch.zeros(1, dtype=torch.int32, device="cuda")
        out, counts = _run(b, None, fill, err=err)
        assert int(err) == bit
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
        with pytest.raises(ValueError, match=dict(evaluate.POINT_ERRORS)[bit][:20]):
            _run(b, None, fill)                                              # without a word the call itself checks
        _run(b, None, fill, err=word)                                        # bits collect, the word is never cleared
    assert int(word) == P.ERR_LABEL | P.ERR_INVERSE | P.ERR_KEEP
    with pytest.raises(ValueError, match="error word 14"):
        evaluate.check_point_error(word)
    # far outside: the values are compared, never used
    b = dict(clean, keep_row=clean["keep_row"].copy(), inverse_map=clean["inverse_map"].copy())
    b["keep_row"][[0, 1, 2]] = (2 ** 31 - 1, -2, -(2 ** 31))
    b["inverse_map"][[5, 6]] = (2 ** 62, -1)
    err = torch.zeros(1, dtype=torch.int32, device="cuda")
    out, counts = _run(b, None, fill, err=err)
    want, want_counts, e = _want(b, None, fill)
    assert int(err) == e == P.ERR_KEEP | P.ERR_INVERSE
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts)
    err.zero_()
    _run(clean, None, fill, err=err)
    assert int(err) == 0
    # shapes and offsets are refused on the host
    with pytest.raises(ValueError, match="vox_off"):
        _run(dict(clean, vox_off=[0, clean["vox_off"][1], clean["vox_off"][2], clean["vox_off"][3] + 1]))
    with pytest.raises(ValueError, match="row_off"):
        _run(dict(clean, row_off=[0, 1500, 1400, 2200]))
    with pytest.raises(ValueError, match="65 scans"):
        evaluate.point_labels(torch.zeros((4, 7), device="cuda"), [0] * 66, [0] * 66, [0] * 65 + [4],
                              torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="classes"):
        evaluate.point_labels(torch.zeros((4, 33), device="cuda"), [0, 0], [0, 0], [0, 4],
                              torch.zeros(0, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"))
    # no records: nothing is launched
    out, counts = evaluate.point_labels(torch.zeros((0, 7), device="cuda"), [0, 0], [0, 0], [0, 0],
                                        torch.zeros(0, dtype=torch.int32, device="cuda"),
                                        torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert out.shape == (0,) and counts is None


# ------------------------------------------------------------------ consistency with the voxel path
def test_point_predictions_at_first_points_equal_the_voxel_path(tmp_path):
    from lidog_amd.data import collate_items
    root, _, lut = P.write_tiny_kitti_tree(str(tmp_path / "kitti"))
    data = scans.FileScans(scans.listing("SemanticKITTI", root, "validation"), lut, keep_raw=True)
    assert len(data) == 3
    items = [data.item(i) for i in range(3)]
    batch = collate_items(items, False)
    coords, labels = batch["coords_int"], batch["source_sem_labels0"]
    v = coords.shape[0]
    logits = _cuda(_logits(v, 7, 9))
    preds, _ = evaluate.confusion(logits, labels, coords, 3)
    recs = evaluate.unpack_predictions(evaluate.pack_predictions(coords, preds, labels, 3), 3)
    pitems = [data.point_item(i) for i in range(3)]
    with pytest.raises(KeyError):
        data.point_item(0)                                                   # handed out once
    pin = evaluate.point_inputs(pitems)
    out, counts = evaluate.point_labels(logits, pin["row_off"], pin["kept_off"], pin["vox_off"], pin["keep_row"],
                                        pin["inverse_map"], labels_raw=pin["labels_raw"], lut=pin["lut"],
                                        label_mask=pin["label_mask"])
    out, keep_row, preds_h = out.cpu().numpy(), pin["keep_row"].cpu().numpy(), preds.cpu().numpy()
    for s in range(3):
        rows = slice(int(pin["row_off"][s]), int(pin["row_off"][s + 1]))
        raw = np.fromfile(data.listings[0].files[s][0], dtype=np.float32)
        assert pitems[s]["rows"] == raw.size // 4 == rows.stop - rows.start
        want_keep, m = P.keep_rows_np(raw, 4, RADIUS)
        assert np.array_equal(keep_row[rows], want_keep) and m == pitems[s]["kept"] < pitems[s]["rows"]
        assert pitems[s]["voxels"] < m                                       # some points share a voxel
        file_row = np.nonzero(want_keep >= 0)[0]                             # kept row -> file row
        first = items[s][0]["sampled_idx"].cpu().numpy()                     # kept row of every voxel's first point
        vox = slice(int(pin["vox_off"][s]), int(pin["vox_off"][s + 1]))
        assert np.array_equal(out[rows][file_row[first]], preds_h[vox])
        lab = labels[vox].cpu().numpy()
        assert np.array_equal(out[rows][file_row[first[lab != -1]]], recs[s][:, 3])     # the dump's predictions
        assert (out[rows][want_keep < 0] == 0).all()
    # and the whole batch against the restatement, raw labels included
    want, want_counts, err = P.point_labels_np(
        logits.cpu().numpy(), pin["row_off"], pin["kept_off"], pin["vox_off"], keep_row, pin["inverse_map"].cpu().numpy(),
        labels_raw=pin["labels_raw"].cpu().numpy(), lut=lut, mask=0xFFFF)
    assert err == 0 and np.array_equal(out, want) and np.array_equal(counts.cpu().numpy(), want_counts)
    assert 0 < want_counts.sum() < (keep_row >= 0).sum()
