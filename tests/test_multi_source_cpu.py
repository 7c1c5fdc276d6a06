"""Two-source training without a GPU: the collated two-source batch, source pairing as MultiBEVSourceDataset, the
one-source batch unchanged, the CLI's --sources / --source-weights and step choice, gradient buckets expecting two
uses per parameter, and the accumulate entry point of the C ABI."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from helpers import REPO

KINDS = ["MinkUNet34BEV", "MinkUNet34", "MinkUNet34IBN", "MinkUNet34Robust"]


def test_two_source_batch_keys_dtypes_and_batch_column():
    from lidog_amd import synth
    b = synth.make_batch([0, 1], "source8k", "cpu", bev_size=9, seeds1=[2], config1="nusc35k")
    for s, n_scans in ((0, 2), (1, 1)):
        c, ci = b[f"source_coordinates{s}"], b["coords_int" if s == 0 else "coords_int1"]
        assert c.dtype == torch.float32 and ci.dtype == torch.int32 and c.shape == ci.shape and c.shape[1] == 4
        assert torch.equal(c, ci.float())
        assert sorted(ci[:, 0].unique().tolist()) == list(range(n_scans))
        assert b[f"source_features{s}"].shape == (c.shape[0], 1) and b[f"source_features{s}"].dtype == torch.float32
        assert b[f"source_sem_labels{s}"].shape == (c.shape[0],) and b[f"source_sem_labels{s}"].dtype == torch.int64
        bev = b[f"source_bev_labels{s}"]
        assert list(bev) == ["block8"] and bev["block8"].shape == (n_scans, 9, 9) and bev["block8"].dtype == torch.int64
    v, _ = synth.scan_voxels(synth.SOURCE1_SEED + 2, "nusc35k")
    assert torch.equal(b["coords_int1"][:, 1:], torch.from_numpy(v))


def test_source1_scans_differ_from_source0_with_the_same_config():
    from lidog_amd import synth
    b = synth.make_batch([0, 1], "source8k", "cpu", seeds1=[0, 1])
    assert b["coords_int"].shape != b["coords_int1"].shape or not torch.equal(b["coords_int"], b["coords_int1"])
    assert not torch.equal(b["source_bev_labels0"]["block8"], b["source_bev_labels1"]["block8"])


def _digest(batch):
    h = hashlib.sha256()
    for k in sorted(batch):
        v = batch[k]["block8"] if isinstance(batch[k], dict) else batch[k]
        h.update(k.encode() + str(v.dtype).encode() + v.contiguous().numpy().tobytes())
    return h.hexdigest()


def test_one_source_batch_is_unchanged():
    """the one-source batch rebuilt from its definition (the collation before two sources existed)"""
    from lidog_amd import synth
    seeds = [3, 4]
    b = synth.make_batch(seeds, "source8k", "cpu", bev_size=11)
    assert sorted(b) == ["coords_int", "source_bev_labels0", "source_coordinates0", "source_features0",
                         "source_sem_labels0"]
    coords, labels = [], []
    for i, s in enumerate(seeds):
        v, l = synth.scan_voxels(s, "source8k")
        coords.append(np.concatenate([np.full((v.shape[0], 1), i, np.int32), v], axis=1))
        labels.append(l)
    coords = torch.from_numpy(np.concatenate(coords))
    bev = torch.from_numpy(np.random.default_rng(1000003 + seeds[0]).integers(-1, 7, (2, 11, 11))).long()
    want = {"source_coordinates0": coords.float(), "source_features0": torch.ones((coords.shape[0], 1)),
            "source_sem_labels0": torch.from_numpy(np.concatenate(labels)).long(),
            "source_bev_labels0": {"block8": bev}, "coords_int": coords}
    assert _digest(b) == _digest(want)


def test_pairing_length_and_fallback_draws_follow_multibevsourcedataset():
    from lidog_amd.train import MultiSynthScans
    d = MultiSynthScans(7, 4, ("source8k", "source8k"), seed=99)
    assert len(d) == 7
    assert sorted(d.perm1.tolist()) == [0, 1, 2, 3]
    pairs = [d.pair(i) for i in range(7)]
    for i, (j0, j1) in enumerate(pairs):
        assert j0 == i                               # i < len(source 0): scan i
        if i < 4:
            assert j1 == d.perm1[i]                  # through the permutation shuffled at construction
        else:
            assert 0 <= j1 < 4                       # past the end: a random scan of source 1
    again = MultiSynthScans(7, 4, ("source8k", "source8k"), seed=99)
    assert [again.pair(i) for i in range(7)] == pairs and np.array_equal(again.perm1, d.perm1)
    other = MultiSynthScans(7, 4, ("source8k", "source8k"), seed=100)
    assert [other.pair(i) for i in range(7)] != pairs or not np.array_equal(other.perm1, d.perm1)
    rev = MultiSynthScans(3, 6, ("source8k", "source8k"), seed=5)
    assert len(rev) == 6 and all(0 <= rev.pair(i)[0] < 3 for i in range(3, 6))
    from lidog_amd import synth
    b = MultiSynthScans(7, 4, ("source8k", "source8k"), seed=99).batch([0, 5], "cpu")
    twin = MultiSynthScans(7, 4, ("source8k", "source8k"), seed=99)
    p = [twin.pair(0), twin.pair(5)]
    assert torch.equal(b["coords_int1"], synth.make_batch([0], "source8k", seeds1=[p[0][1], p[1][1]])["coords_int1"])
    assert torch.equal(b["coords_int"], synth.make_batch([0, 5], "source8k")["coords_int"])


def test_more_than_two_sources_is_not_implemented():
    from lidog_amd.train import MultiSynthScans, build_step
    with pytest.raises(NotImplementedError):
        MultiSynthScans(2, 2, ("source8k",) * 3)
    with pytest.raises(NotImplementedError):
        build_step(torch.nn.Linear(2, 2), "MinkUNet34", num_sources=3)


@pytest.mark.parametrize("kind", KINDS)
def test_cli_sources_pick_the_two_source_step(kind):
    from lidog_amd.train import build_model, build_step, parse_args
    from lidog_amd.trainer import LiDOGStep, RobustStep, SourceStep
    a = parse_args(["--model", kind, "--sources", "kitti120k", "nusc35k", "--source-weights", "0.3", "0.7"])
    assert a.sources == ["kitti120k", "nusc35k"] and a.source_weights == [0.3, 0.7]
    _, step, _ = build_step(build_model(kind, device="cpu"), kind, source_weights=tuple(a.source_weights),
                            num_sources=len(a.sources))
    want = {"MinkUNet34BEV": LiDOGStep, "MinkUNet34Robust": RobustStep}.get(kind, SourceStep)
    assert type(step) is want and step.num_sources == 2 and tuple(step.w) == (0.3, 0.7)
    assert step.opt.buckets.uses == 2
    plain = parse_args(["--model", kind])
    assert plain.sources is None and list(plain.source_weights) == [0.5, 0.5]
    _, one, _ = build_step(build_model(kind, device="cpu"), kind)
    assert type(one) is want and one.num_sources == 1 and one.opt.buckets.uses == 1


def test_validation_keys_are_unique_source_names():
    from lidog_amd.train import source_names
    assert source_names(["kitti120k", "nusc35k"]) == ["kitti120k", "nusc35k"]
    assert source_names(["kitti120k", "kitti120k"]) == ["kitti120k:0", "kitti120k:1"]


def test_buckets_wait_for_both_uses():
    """the hook path's countdown with two uses per parameter (a one-rank stand-in for an active GradientBuckets)"""
    from lidog_amd.optim import FlatParams, GradientBuckets
    net = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
    flat = FlatParams(net)
    gb = GradientBuckets(flat)
    assert not gb.active and gb.uses == 1
    gb.active = True                       # bucket bookkeeping without a process group
    gb.index_of = {id(p): i for i, p in enumerate(flat.params)}
    gb.bucket_of = {id(p): 0 for p in flat.params}
    gb.pending0 = [len(flat.params)]
    gb.slices = [(0, flat.total)]
    gb.pending = np.array(gb.pending0, dtype=np.int32)
    gb.c_uses = np.zeros(len(flat.params), dtype=np.int32)
    reduced = []
    gb._reduce = reduced.append
    for p in flat.params:
        p.register_post_accumulate_grad_hook(gb._hook)
    gb.set_uses(2)
    assert gb.pending.tolist() == [2 * len(flat.params)]
    gb.c_uses[0] = 1                       # the executor counted parameter 0 once in C
    gb.pending[0] -= 1
    flat.zero_grad()
    x = torch.randn(3, 4)
    (net(x).sum() + net(x).sum()).backward()   # every hook fires once, after both uses are summed
    assert gb.pending.tolist() == [0] and reduced == [0]
    with pytest.raises(NotImplementedError):
        gb.set_uses(3)


def test_accumulate_symbol_is_exported_and_declared():
    from lidog_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "lidog_grad_accumulate")
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    assert re.search(r"int lidog_grad_accumulate\(const int64_t \*segs, int32_t n_segs, void \*stream\);", header)
    assert _lib.SIGNATURES["lidog_grad_accumulate"] == [_lib._p, _lib._i32, _lib._p]
    assert lib.lidog_grad_accumulate.argtypes == [_lib._p, _lib._i32, _lib._p]
