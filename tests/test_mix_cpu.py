"""PointCutMix / CoSMix without a GPU: the host draws replay the reference's recorded draws (G11), the command line, the
C ABI of the mixing kernels, and per-item draws that do not depend on how the items are batched."""
import os
import re

import numpy as np
import pytest
import torch

import mix_ref
from helpers import REPO
from lidog_amd import data
from lidog_amd.data import cosmix_merge, draw_cells, draw_classes, draw_source, pointcutmix_merge
from lidog_amd.train import MixedSynthScans, parse_args

G11 = mix_ref.load_g11()
MIX_SYMBOLS = ("lidog_mix_histogram", "lidog_mix_split_ws", "lidog_mix_split", "lidog_mix_gather")


def _ids(cases):
    return [f"{c['method']}-{c['config0']}-{c['config1']}-seed{c['seed']}{'-raises' if c['outcome'] == 'raises' else ''}"
            for c, _ in cases]


@pytest.mark.parametrize("case", G11, ids=_ids(G11))
@pytest.mark.parametrize("global_state", [True, False], ids=["np.random", "RandomState"])
def test_host_draws_replay_the_reference(case, global_state):
    c, arr = case
    if global_state:
        np.random.seed(c["seed"])
        rng = np.random
    else:
        rng = np.random.RandomState(c["seed"])
    assert draw_source(rng) == c["source"]
    if c["method"] == "pointcutmix":
        if c["outcome"] == "raises":
            with pytest.raises(ValueError):
                draw_cells(rng, arr["counts"])
            return
        assert draw_cells(rng, arr["counts"]).tolist() == c["choice"]
        return
    w = arr["w1"] if c["source"] else arr["w0"]
    classes, subs = draw_classes(rng, arr["counts"], w, c["sub_p"])
    assert classes.tolist() == c["choice"]
    if c["sub_p"] is None:
        assert c["subs"] == [] and [s.tolist() for s in subs] == [list(range(arr["counts"][k])) for k in classes]
    else:
        assert [[len(s), mix_ref.digest(np.asarray(s, dtype=np.int64))] for s in subs] == c["subs"]


def test_g11_covers_the_edge_cases():
    kinds = {(c["method"], c["config0"], c["outcome"], c["sub_p"], c["one_class"]) for c, _ in G11}
    assert ("pointcutmix", "source8k", "raises", 0.8, False) in kinds
    assert ("cosmix", "source8k", "ok", None, False) in kinds
    assert ("cosmix", "source8k", "ok", 0.8, True) in kinds
    for cfg in ("kitti120k", "nusc35k", "source8k"):
        assert all((m, cfg, "ok", 0.8, False) in kinds for m in ("pointcutmix", "cosmix"))
    # both draws of the source hit the raising and the empty cases
    assert {c["source"] for c, _ in G11 if c["outcome"] == "raises"} == {0, 1}
    assert {c["source"] for c, _ in G11 if c["one_class"]} == {0, 1}
    assert all(c["choice"] == [] for c, _ in G11 if c["one_class"])
    assert os.path.getsize(mix_ref.G11) < 1 << 20


def test_cosmix_refuses_augmentations_and_cpu_tensors():
    s = {"coordinates": torch.zeros((4, 3), dtype=torch.int32), "features": torch.ones((4, 1)),
         "sem_labels": torch.zeros(4, dtype=torch.int64)}
    with pytest.raises(NotImplementedError):
        cosmix_merge(s, s, class_weights=(np.ones(7), np.ones(7)), augmentations=lambda c: c)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        cosmix_merge(s, s, class_weights=(np.ones(7), np.ones(7)))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        pointcutmix_merge(s, s)


# ------------------------------------------------------------------ command line
def test_cli_defaults_are_unchanged():
    a = parse_args([])
    assert a.mix is None and a.sources is None and a.sub_p == 0.8 and a.model == "MinkUNet34BEV" and not a.mix3d


@pytest.mark.parametrize("method", MixedSynthScans.METHODS)
def test_cli_mix_takes_config_twice_and_the_source_step(method):
    from lidog_amd.train import build_model, build_step
    from lidog_amd.trainer import SourceStep
    a = parse_args(["--model", "MinkUNet34", "--mix", method, "--config", "nusc35k", "--sub-p", "0.5"])
    assert a.mix == method and a.sources == ["nusc35k", "nusc35k"] and a.sub_p == 0.5
    b = parse_args(["--model", "MinkUNet34IBN", "--mix", method, "--sources", "kitti120k", "source8k"])
    assert b.sources == ["kitti120k", "source8k"]
    model = build_model("MinkUNet34", device="cpu")
    _, step, _ = build_step(model, "MinkUNet34", num_sources=MixedSynthScans.num_sources)
    assert type(step) is SourceStep and step.num_sources == 1


@pytest.mark.parametrize("argv", [["--mix", "cosmix"], ["--model", "MinkUNet34Robust", "--mix", "cosmix"],
                                  ["--model", "MinkUNet34", "--mix", "pointcutmix", "--mix3d"],
                                  ["--model", "MinkUNet34", "--mix", "raycast"]])
def test_cli_mix_refusals(argv, capsys):
    with pytest.raises(SystemExit):
        parse_args(argv)


# ------------------------------------------------------------------ C ABI
def test_mix_symbols_are_declared_bound_and_exported():
    from lidog_amd import _lib, build
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    lib = __import__("ctypes").CDLL(build.build())
    for name in MIX_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "mix.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9


# ------------------------------------------------------------------ per-item draws
def _recording(ds, log):
    def merge(s0, s1, rng):
        log.append((int(s0["coordinates"].shape[0]), int(s1["coordinates"].shape[0]), draw_source(rng),
                    int(rng.randint(1 << 30))))
        return {"coordinates": s0["coordinates"], "features": s0["features"], "sem_labels": s0["sem_labels"]}
    ds.merge = merge


def test_per_item_draws_do_not_depend_on_the_batching():
    ds = MixedSynthScans(4, 4, ("source8k", "source8k"), method="pointcutmix", seed=7)
    whole, split = [], []
    _recording(ds, whole)
    ds.set_epoch(1)
    b = ds.batch([0, 1, 2, 3], "cpu")
    _recording(ds, split)
    for part in ([2], [0, 3], [1]):
        ds.batch(part, "cpu")
    order = {i: k for k, i in enumerate([2, 0, 3, 1])}
    assert [split[order[i]] for i in range(4)] == whole
    assert len({w[3] for w in whole}) == 4
    assert b["coords_int"].dtype == torch.int32 and b["coords_int"][:, 0].unique().tolist() == [0, 1, 2, 3]
    assert set(b) == {"coords_int", "source_coordinates0", "source_features0", "source_sem_labels0"}
    again = []
    _recording(ds, again)
    ds.set_epoch(2)
    ds.batch([0, 1, 2, 3], "cpu")
    assert [a[3] for a in again] != [w[3] for w in whole]      # a new epoch, new mixes
    ds2 = MixedSynthScans(4, 4, ("source8k", "source8k"), method="pointcutmix", seed=7)
    resumed = []
    _recording(ds2, resumed)
    ds2.set_epoch(1)
    ds2.batch([0, 1, 2, 3], "cpu")
    assert resumed == whole                                    # a fresh run (a resume) draws the same


def test_cosmix_class_weights_count_the_training_scans():
    from lidog_amd import synth
    from lidog_amd.train import source_class_counts
    ds = MixedSynthScans(2, 3, ("source8k", "nusc35k"), method="cosmix", seed=1)
    w0, w1 = ds.class_weights
    exp0 = sum(np.bincount(synth.scan_voxels(j, "source8k")[1] + 1, minlength=8)[1:] for j in range(2))
    exp1 = sum(np.bincount(synth.scan_voxels(synth.SOURCE1_SEED + j, "nusc35k")[1] + 1, minlength=8)[1:]
               for j in range(3))
    assert w0.tolist() == exp0.tolist() and w1.tolist() == exp1.tolist()
    assert source_class_counts("source8k", [0, 1]).tolist() == exp0.tolist()
    assert ds.voxel == 0.1 and data.merge_stream is not None
