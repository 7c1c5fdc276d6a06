"""Host-side pieces of the opt-in bf16 training mode (lidog_amd/precision.py, lidog_amd/train.py, include/lidog_amd.h):
the command line, precision.resolve, the layout arithmetic of the two operand tables, the weight-gradient kernel's slab
count, and the declared symbols.  No GPU."""
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_precision_flag_is_absent_by_default_and_read_by_its_accessor():
    from lidog_amd.train import parse_args, precision_of, val_precision_of
    a = parse_args([])
    assert not hasattr(a, "precision"), "--precision is a late flag: default=argparse.SUPPRESS"
    assert precision_of(a) is None and val_precision_of(a) == "fp32"
    a = parse_args(["--precision", "bf16"])
    assert a.precision == "bf16" and precision_of(a) == "bf16" and val_precision_of(a) == "fp32"
    a = parse_args(["--precision", "fp32", "--val-precision", "bf16"])
    assert precision_of(a) == "fp32" and val_precision_of(a) == "bf16"       # independent of each other
    with pytest.raises(SystemExit):
        parse_args(["--precision", "int8"])


def test_resolve():
    from lidog_amd import precision
    assert precision.resolve(None) is None and precision.resolve("fp32") is False and precision.resolve("bf16") is True
    for bad in ("int8", "BF16", "fp16", 16, True):
        with pytest.raises(ValueError, match="precision"):
            precision.resolve(bad)


def test_fit_and_steps_refuse_an_unknown_precision_before_building_anything():
    from lidog_amd.train import Fit, build_step
    from lidog_amd.trainer import SourceStep
    with pytest.raises(ValueError, match="precision"):
        Fit(model_kind="MinkUNet34", precision="int8", device="cpu")
    with pytest.raises(ValueError, match="precision"):
        build_step(None, precision="int8")
    with pytest.raises(ValueError, match="precision"):
        SourceStep(None, None, precision="fp16")


def test_more_than_one_rank_is_refused(monkeypatch):
    import torch.distributed as dist
    from lidog_amd import precision
    precision.check_single_rank()           # no process group: fine
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 1)
    precision.check_single_rank()
    monkeypatch.setattr(dist, "get_world_size", lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match="executor"):
        precision.check_single_rank()


def test_table_layouts():
    """offsets in bf16 elements and first 32 x 32 tiles of both tables: the forward operands back to back, then the
    packs of the transposed kernels (source `Cin` = Cout), continuing the same element and tile ranges"""
    from lidog_amd import precision
    shapes = [(27, 32, 64), (8, 128, 96), (1, 96, 32), (27, 384, 256)]
    fwd, dgrad, elems, tiles = precision.training_layout(shapes)
    sizes = [K * a * b for K, a, b in shapes]
    ntiles = [K * (a // 32) * (b // 32) for K, a, b in shapes]
    assert ntiles == [27 * 2, 8 * 12, 3, 27 * 96]
    off = t = 0
    for row, (K, Cin, Cout), n, nt in zip(fwd, shapes, sizes, ntiles):
        assert row == (off, K, Cin, Cout, t)
        off, t = off + n, t + nt
    assert off == sum(sizes) and t == sum(ntiles)
    for row, (K, Cin, Cout), n, nt in zip(dgrad, shapes, sizes, ntiles):
        assert row == (off, K, Cout, Cin, t)        # the transposed kernel is the source: its `Cin` is Cout
        off, t = off + n, t + nt
    assert (elems, tiles) == (2 * sum(sizes), 2 * sum(ntiles)) == (off, t)
    # the evaluation table is the first half
    assert precision.table_layout(shapes) == (fwd, sum(sizes), sum(ntiles))
    assert precision.table_layout([]) == ([], 0, 0)
    # every table's tile range is contiguous and ascending: the pack kernel finds a tile's matrix by bisection
    firsts = [r[4] for r in fwd + dgrad]
    assert firsts == sorted(firsts) and len(set(firsts)) == len(firsts)


def test_wgrad_bf16_slab_arithmetic():
    """one slab per work item, two where the kernel has at most two MFMA tiles per workgroup (the two k = 16 steps of a
    chunk go to two groups of waves); 0 for a shape the kernel does not take.  Host arithmetic: no device needed."""
    from lidog_amd import _lib
    L = _lib.load()
    tile = lambda c: 4 if c % 128 == 0 else 3 if c % 96 == 0 else 2 if c % 64 == 0 else 1   # noqa: E731
    for Cin in (32, 64, 96, 128, 192, 256, 384):
        for Cout in (32, 64, 96, 128, 256):
            per = 2 if tile(Cin) * tile(Cout) <= 2 else 1
            for n in (0, 1, 7, 2048):
                assert L.lidog_sconv_wgrad_bf16_slabs(Cin, Cout, n) == per * n, (Cin, Cout, n)
    for Cin, Cout in ((1, 32), (96, 7), (33, 32), (0, 32), (32, -32)):
        assert L.lidog_sconv_wgrad_bf16_slabs(Cin, Cout, 5) == 0
    assert L.lidog_sconv_wgrad_bf16_slabs(32, 32, -1) == 0


def test_wgrad_chunk_reads_the_bf16_kernels_own_slots(monkeypatch):
    """me._wgrad_chunk(bf16=True) fits a launch to the slots of lidog_sconv_wgrad_bf16, not to the fp32 kernel's"""
    import numpy as np
    import lidog_amd.me as ME
    rng = np.random.default_rng(3)
    cnt = (352_000 * np.concatenate([rng.uniform(0.05, 0.4, 13), [1.0], rng.uniform(0.05, 0.4, 13)])).astype(np.int64)
    k_off = np.concatenate([[0], np.cumsum(cnt)])
    items = lambda chunk: int(np.sum((cnt + chunk - 1) // chunk))   # noqa: E731
    monkeypatch.setattr(ME, "_wgrad_slots", lambda cin, cout, bf16=False: 1280 if bf16 else 768)
    monkeypatch.setattr(ME, "_WGRAD_FIT", 1)
    fp32, bf16 = ME._wgrad_chunk(k_off, 128, 128), ME._wgrad_chunk(k_off, 128, 128, bf16=True)
    assert fp32 % 32 == 0 and bf16 % 32 == 0 and fp32 != bf16
    assert items(fp32) <= 3 * 768 < items(fp32 - 32)            # 2 048 / 768 = 2.67 -> three whole rounds
    assert items(bf16) <= 2 * 1280 < items(bf16 - 32)           # 2 048 / 1 280 = 1.6 -> two whole rounds
    monkeypatch.setattr(ME, "_WGRAD_FIT", 0)                    # no fitting: the same cut for both
    assert ME._wgrad_chunk(k_off, 128, 128) == ME._wgrad_chunk(k_off, 128, 128, bf16=True)


def test_new_symbols_are_declared_and_bound():
    from lidog_amd import _lib
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    declared = set(re.findall(r"\b(lidog_[a-z0-9_]+)\s*\(", header))
    for name in ("lidog_sconv_wgrad_bf16", "lidog_sconv_wgrad_bf16_slabs", "lidog_sconv_wgrad_bf16_slots"):
        assert name in declared and name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["lidog_sconv_wgrad_bf16"] == _lib.SIGNATURES["lidog_sconv_wgrad"]
