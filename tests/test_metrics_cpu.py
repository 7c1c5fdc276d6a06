"""Per-step training metrics without a GPU: the ABI of lidog_train_confusion, iou_from_counts against fixture G17
(sklearn's jaccard_score, the confusion-matrix Jaccard of the LiDOG trainers, torch.unique), the mean over ranks, the
keys of every step class, the metrics file and the command-line flag."""
import ctypes
import os

import numpy as np
import pytest
import torch

import metrics_ref as M
from helpers import REPO


def test_train_confusion_symbol_exported_bound_and_refuses_bad_arguments():
    from lidog_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    name = "lidog_train_confusion"
    assert hasattr(lib, name) and name in _lib.SIGNATURES and f"{name}(" in header
    assert len(_lib.SIGNATURES[name]) == 9
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9          # an additive entry: the version stays
    assert "trainstats.hip" in build.SOURCES
    lib.lidog_last_error.restype = ctypes.c_char_p
    i64, i32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    fn = lib.lidog_train_confusion

    def table(ns, pointer=1 << 20):
        k = len(ns)
        return (vp * k)(*[pointer] * k), (vp * k)(*[pointer] * k), (i64 * k)(*ns)

    # every argument error is refused on the host with status 2, before any launch
    lg, lb, n = table([10])
    assert fn(lg, lb, n, i32(1), i32(0), i64(-1), vp(1 << 20), vp(1 << 20), vp()) == 2
    assert b"0 classes" in lib.lidog_last_error()
    assert fn(lg, lb, n, i32(1), i32(33), i64(-1), vp(1 << 20), vp(1 << 20), vp()) == 2
    assert b"33 classes" in lib.lidog_last_error()
    assert fn(lg, lb, n, i32(0), i32(7), i64(-1), vp(1 << 20), vp(1 << 20), vp()) == 2
    assert b"0 segments" in lib.lidog_last_error()
    lg9, lb9, n9 = table([1] * 9)
    assert fn(lg9, lb9, n9, i32(9), i32(7), i64(-1), vp(1 << 20), vp(1 << 20), vp()) == 2
    assert b"9 segments" in lib.lidog_last_error()
    lg, lb, n = table([5, -1])
    assert fn(lg, lb, n, i32(2), i32(7), i64(-1), vp(1 << 20), vp(1 << 20), vp()) == 2
    assert b"segment 1: n = -1" in lib.lidog_last_error()
    lg, lb, n = table([0, 5], pointer=None)                      # null is fine for the empty segment only
    assert fn(lg, lb, n, i32(2), i32(7), i64(-1), vp(1 << 20), vp(1 << 20), vp()) == 2
    assert b"segment 1: null pointer" in lib.lidog_last_error()
    assert fn(vp(), vp(), vp(), i32(1), i32(7), i64(-1), vp(1 << 20), vp(1 << 20), vp()) == 2
    lg, lb, n = table([5])
    assert fn(lg, lb, n, i32(1), i32(7), i64(-1), vp(), vp(), vp()) == 2
    # nothing to count: no launch, no pointer is read
    lg, lb, n = table([0, 0], pointer=None)
    assert fn(lg, lb, n, i32(2), i32(7), i64(-1), vp(), vp(), vp()) == 0


@pytest.fixture(scope="module")
def g17():
    return np.load(M.G17)


@pytest.mark.parametrize("name", list(M.CASES))
def test_iou_from_counts_equals_the_reference_formulas(g17, name):
    from lidog_amd.metrics import iou_from_counts, mean_present
    logits, labels = torch.from_numpy(g17[f"{name}/logits"]), g17[f"{name}/labels"]
    again = M.make_case(name, int(g17[f"{name}/seed"]))
    assert tuple(logits.shape) == tuple(M.CASES[name]["shape"]) and np.array_equal(again[1].numpy(), labels)
    counts = torch.from_numpy(M.host_counts(logits, labels))
    assert int(counts.sum()) == labels.size
    for count_ignored, key in ((True, "all"), (False, "valid")):
        iou, present, occ = iou_from_counts(counts, count_ignored)
        assert iou.dtype == torch.float64 and iou.shape == (M.C,)
        np.testing.assert_allclose(iou.numpy(), g17[f"{name}/iou_{key}"], rtol=0, atol=1e-15)
        assert np.flatnonzero(present.numpy()).tolist() == g17[f"{name}/present"].tolist()
        assert occ.numpy()[present.numpy()].tolist() == g17[f"{name}/occurs"].tolist()
        assert int(occ[~present].sum()) == 0
        assert abs(float(mean_present(iou, present)) - float(g17[f"{name}/mean_{key}"])) <= 1e-15
    if name == "all_ignored":
        assert not present.any() and float(mean_present(iou, present)) == 0.0
    if name == "absent_class":
        assert present.tolist() == [True, True, True, False, True, False, True]
        # an absent class that is predicted: union > 0, IoU 0, and the ignored rows enlarge unions only when counted
        assert (iou_from_counts(counts, True)[0] <= iou_from_counts(counts, False)[0]).all()
    # batched: leading dimensions pass through
    both = torch.stack([counts, counts * 2])
    iou2, present2, occ2 = iou_from_counts(both, True)
    assert iou2.shape == (2, M.C) and torch.equal(iou2[0], iou2[1]) and torch.equal(occ2[1], 2 * occ2[0])
    with pytest.raises(ValueError):
        iou_from_counts(torch.zeros(7, 7, dtype=torch.int64), True)


def _layout(step="SourceStep", sources=("kitti120k",), levels=("block8",)):
    from lidog_amd import trainer
    from lidog_amd.metrics import MetricLayout
    return MetricLayout.for_step(getattr(trainer, step), sources, levels)


def test_keys_of_every_step_class_one_and_two_sources():
    from lidog_amd.evaluate import CLASS_NAMES
    lay = _layout("SourceStep")
    per_class = [f"training/kitti120k/{n}_{k}" for k in ("iou", "count") for n in CLASS_NAMES]
    assert lay.keys == per_class + ["training/kitti120k/source_iou0", "training/kitti120k/total_loss",
                                    "training/kitti120k/sem_loss0", "training/lr"]
    assert lay.count_ignored and lay.segments == [(0, None)]
    lay = _layout("RobustStep", ("a", "b"))
    assert lay.segments == [(0, None), (1, None)] and lay.count_ignored
    assert lay.keys[-6:] == ["training/a/total_loss", "training/a/sem_loss0", "training/b/sem_loss1",
                             "training/a/aux_loss0", "training/b/aux_loss1", "training/lr"]
    assert "training/b/source_iou1" in lay.keys and "training/b/road_iou" in lay.keys
    lay = _layout("LiDOGStep")
    assert lay.segments == [(0, None), (0, "block8")] and not lay.count_ignored
    assert lay.keys[15:30] == [f"training/kitti120k/{n}_{k}_bev_block8" for k in ("iou", "count") for n in CLASS_NAMES] + \
        ["training/kitti120k/source_iou_bev0_block8"]
    assert lay.keys[-4:] == ["training/kitti120k/total_loss", "training/kitti120k/sem_loss0",
                             "training/kitti120k/bev_loss0", "training/lr"]
    lay = _layout("LiDOGStep", ("kitti120k", "nusc35k"), ("block4", "block8"))
    assert len(lay.segments) == 6 and "training/nusc35k/source_iou_bev1_block4" in lay.keys
    assert lay.keys[-6:-1] == ["training/kitti120k/total_loss", "training/kitti120k/sem_loss0",
                               "training/nusc35k/sem_loss1", "training/kitti120k/bev_loss0", "training/nusc35k/bev_loss1"]
    assert len(set(lay.keys)) == len(lay.keys) == 6 * 15 + 6
    with pytest.raises(ValueError):
        _layout("LiDOGStep", ("a", "b"), ("l1", "l2", "l3", "l4"))        # 10 tensors in one launch
    with pytest.raises(ValueError):
        _layout("SourceStep", ("a", "a"))


def _rank_counts(seed, absent=()):
    """made-up counts [1 step, 1 segment, 8, 7] of one rank; `absent`: classes that do not occur in its labels"""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 40, (1, 1, M.C + 1, M.C), generator=g)
    for a in absent:
        c[0, 0, a + 1] = 0
    return c


@pytest.mark.parametrize("world", [2, 4])
def test_rank_mean_is_the_mean_over_the_ranks_where_a_key_is_present(world):
    from lidog_amd.metrics import iou_from_counts, mean_present
    lay = _layout("SourceStep")
    # class 3 is labelled on rank 0 only, class 5 on no rank
    counts = [_rank_counts(10 + r, absent=(5,) if r == 0 else (3, 5)) for r in range(world)]
    scalars = [torch.tensor([[0.5 + r, 0.25 * (r + 1), 0.01]], dtype=torch.float64) for r in range(world)]
    packed = sum(lay.pack(c, s) for c, s in zip(counts, scalars))        # what the one all_reduce leaves on every rank
    assert packed.shape == (1, 2 * len(lay.keys))
    values, present = lay.rank_mean(packed)
    rec = lay.records(values, present, [7], [2])[0]
    per_rank = [iou_from_counts(c[0, 0], True) for c in counts]
    for cls, name in enumerate(lay.class_names):
        have = [r for r in range(world) if bool(per_rank[r][1][cls])]
        if not have:
            assert f"training/kitti120k/{name}_iou" not in rec and f"training/kitti120k/{name}_count" not in rec
            continue
        want = sum(float(per_rank[r][0][cls]) for r in have) / len(have)
        assert abs(rec[f"training/kitti120k/{name}_iou"] - want) <= 1e-15
        want = sum(int(per_rank[r][2][cls]) for r in have) / len(have)
        assert abs(rec[f"training/kitti120k/{name}_count"] - want) <= 1e-12
    assert "training/kitti120k/sidewalk_iou" in rec and "training/kitti120k/manmade_iou" not in rec
    assert rec["training/kitti120k/sidewalk_iou"] == float(per_rank[0][0][3])          # rank 0's value, not a quarter of it
    want = sum(float(mean_present(i, p)) for i, p, _ in per_rank) / world
    assert abs(rec["training/kitti120k/source_iou0"] - want) <= 1e-15
    assert abs(rec["training/kitti120k/total_loss"] - sum(0.5 + r for r in range(world)) / world) <= 1e-15
    assert abs(rec["training/lr"] - 0.01) <= 1e-17 and rec["step"] == 7 and rec["training/epoch"] == 2
    # one rank: the values themselves, counts as integers
    v1, p1 = lay.rank_mean(lay.pack(counts[0], scalars[0]))
    r1 = lay.records(v1, p1, [1], [0])[0]
    assert r1["training/kitti120k/vehicle_count"] == int(per_rank[0][2][0]) and isinstance(
        r1["training/kitti120k/vehicle_count"], int)
    with pytest.raises(ValueError):
        lay.rank_mean(packed[:, :-1])


def test_metrics_writer_round_trip(tmp_path):
    from lidog_amd.metrics import MetricsWriter
    path = str(tmp_path / "run" / "metrics.jsonl")
    w = MetricsWriter(path)
    assert not os.path.exists(path)                                   # the file appears with the first record
    recs = [{"step": 2, "training/kitti120k/road_iou": 0.1 + 0.2, "training/kitti120k/road_count": 12, "training/lr": 1e-3,
             "training/epoch": 0},
            {"step": 4, "validation/kitti120k/sem_loss": 0.75, "validation/epoch": 0}]
    for r in recs:
        w.write(r)
    assert MetricsWriter.read(path) == recs                           # floats survive bit for bit
    MetricsWriter(path).write({"step": 6})                            # a resumed run appends
    assert [r["step"] for r in MetricsWriter.read(path)] == [2, 4, 6]
    assert len(open(path).read().splitlines()) == 3


def test_log_every_n_steps_flag_defaults_to_off():
    import inspect
    from lidog_amd import train
    # off unless given; as the other late flags it has no attribute then (the driver reads it with getattr)
    assert getattr(train.parse_args([]), "log_every_n_steps", 0) == 0
    assert train.parse_args(["--log-every-n-steps", "50"]).log_every_n_steps == 50
    assert inspect.signature(train.Fit.__init__).parameters["log_every_n_steps"].default == 0
    assert train.Trainer is train.Fit
    from lidog_amd import trainer
    assert trainer._Step.metrics is None
    assert train.training_source_names(M.Scenes(2), 1) == ["scenes"]
    assert train.training_source_names(train.MultiSynthScans(2, 2, ("kitti120k", "kitti120k")), 2) == \
        ["kitti120k:0", "kitti120k:1"]
    assert train.training_source_names(object(), 2) == ["source0", "source1"]
