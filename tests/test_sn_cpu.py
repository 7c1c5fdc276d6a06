"""The SN car-size scaling baseline without a GPU: the G12 fixture is strong enough to tell a wrong kernel, the host half
of the statistics turns the recorded integer boxes into the recorded float32 dimensions bit for bit, the scale factors and
the per-item draws replay, the scaled dataset does not depend on the batching, the command line, the C ABI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sn_ref
from helpers import REPO
from lidog_amd import data, synth
from lidog_amd.train import ScaledSynthScans, SynthDataset, parse_args

META, G12 = sn_ref.load_g12()
SN_SYMBOLS = ("lidog_dbscan_ws", "lidog_dbscan", "lidog_cluster_boxes", "lidog_sn_scale_coords")


def _clustered(rec):
    return [s for s in rec["scans"] if s["clustered"]]


# ------------------------------------------------------------------ the fixture
def test_g12_is_strong_enough():
    assert os.path.getsize(sn_ref.G12) < 1 << 20
    lattice = sn_ref.lattice_cases(G12)
    assert len(lattice) >= 40 and sum(flag for _, _, flag in lattice) >= 10
    assert set(META["edge"]) >= {"n9", "one_cell", "noise", "border_two_clusters"}
    ok = [r for r in META["stats"] if r["outcome"] == "ok"]
    assert [r for r in META["stats"] if r["outcome"] == "raises"]
    for r in ok:
        assert sum(s["kept"] for s in _clustered(r)) >= 3, r["dataset"]
    scans = [s for r in META["stats"] for s in r["scans"]]
    assert any(s["clustered"] and s["too_small"] for s in scans) and any(s["clustered"] and s["wrong_shape"] for s in scans)
    assert any(not s["clustered"] for s in scans)
    assert any(s["clustered"] and s["noise"] for s in scans)
    for cfg in ("kitti120k_cars", "nusc35k_cars"):
        seen = {(r["dataset"], s["scan"]) for r in META["stats"] if sn_ref.DATASETS[r["dataset"]][0] == cfg
                for s in _clustered(r)}
        assert len(seen) >= 4, cfg
    assert {(len(c["sources"]), len(c["targets"])) for c in META["scaling"]} == {(1, 1), (1, 2), (2, 2)}
    parts = [p for it in META["items"] for p in it["parts"]]
    assert any(p["rows"] < p["rows_in"] for p in parts) and any(p["rows"] == p["rows_in"] for p in parts)
    assert {it["kind"] for it in META["items"]} == {"single", "multi"}


def test_flagged_lattice_cases_tell_the_integer_predicate_apart():
    """the restatement with sklearn's float64 predicate gives the recorded labels; with d^2 <= 100 it does not on the
    flagged cases, and does on the others"""
    for coords, labels, flag in sn_ref.lattice_cases(G12):
        np.testing.assert_array_equal(sn_ref.dbscan_np(coords), labels)
        assert np.array_equal(sn_ref.dbscan_np(coords, integer=True), labels) != flag


def test_edge_cases_restated():
    cases = sn_ref.edge_cases()
    for name in META["edge"]:
        np.testing.assert_array_equal(sn_ref.dbscan_np(cases[name]), G12[f"edge_{name}_labels"], err_msg=name)
    assert (G12["edge_n9_labels"] == -1).all() and (G12["edge_one_cell_labels"] == 0).all()
    assert (G12["edge_noise_labels"] == -1).sum() == 5
    lab = G12["edge_border_two_clusters_labels"]
    assert lab[0] == 0 and set(lab[31:].tolist()) == {1}


# ------------------------------------------------------------------ statistics: the host half
@pytest.mark.parametrize("k", range(len(META["stats"])), ids=[f"{r['dataset']}-seed{r['seed']}" for r in META["stats"]])
@pytest.mark.parametrize("global_state", [True, False], ids=["np.random", "RandomState"])
def test_host_half_of_average_dims_replays_the_reference(k, global_state):
    rec = META["stats"][k]
    if global_state:
        np.random.seed(rec["seed"])
        rng = np.random
    else:
        rng = np.random.RandomState(rec["seed"])
    assert data.draw_scans(rng, META["n_scans"]).tolist() == rec["drawn"]
    name = sn_ref.DATASETS[rec["dataset"]][2]
    min_pts, min_car_pts = data.sn_thresholds(name)
    assert (min_pts, min_car_pts) == ((2000, 300) if name == "NuScenesDataset" else (5000, 1000))
    rows = []
    for s in rec["scans"]:
        assert s["clustered"] == (s["car_voxels"] > min_pts)
        if not s["clustered"]:
            continue
        j = s["slot"]
        counts, lo, hi = G12[f"s{k}_{j}_counts"], G12[f"s{k}_{j}_lo"], G12[f"s{k}_{j}_hi"]
        kept = data.box_dims(counts, lo, hi, META["voxel"], min_car_pts)
        assert len(kept) == s["kept"] and int((counts <= min_car_pts).sum()) == s["too_small"]
        rows += kept
    if rec["outcome"] == "raises":
        assert not rows
        with pytest.raises(ValueError):
            data.mean_dims(rows)
        return
    got = np.concatenate(rows, axis=0)
    assert got.dtype == np.float32 and got.tobytes() == G12[f"s{k}_rows"].tobytes()
    result = data.mean_dims(rows)
    assert result.dtype == np.float32 and result.tobytes() == G12[f"s{k}_result"].tobytes()


def test_boxes_restated_equal_the_recorded_boxes():
    rec = META["stats"][0]
    s = _clustered(rec)[0]
    car = sn_ref.car_voxels(rec["dataset"], s["scan"])
    labels = G12[f"s0_{s['slot']}_labels"].astype(np.int64)
    assert car.shape[0] == s["car_voxels"] == labels.shape[0] and sn_ref.digest(labels.astype(np.int16)) == s["labels_sha1"]
    counts, lo, hi = sn_ref.boxes_np(car, labels)
    np.testing.assert_array_equal(counts, G12[f"s0_{s['slot']}_counts"])
    np.testing.assert_array_equal(lo, G12[f"s0_{s['slot']}_lo"])
    np.testing.assert_array_equal(hi, G12[f"s0_{s['slot']}_hi"])


def test_scaling_params_equal_the_reference(tmp_path):
    ok = {(r["dataset"]): G12[f"s{k}_result"] for k, r in enumerate(META["stats"]) if r["outcome"] == "ok"}
    s, t, u = ok["kitti"], ok["nusc"], ok["kitti_b"]
    out = data.scaling_params([s, u], [t, u, s])
    assert len(out) == 2 and all(a.dtype == np.float32 and a.shape == (3, 3) for a in out)
    for a, src in zip(out, (s, u)):
        for row, tgt in zip(a, (t, u, s)):
            assert row.tobytes() == (tgt / src).astype(np.float32).tobytes()
    assert (out[1][1] == 1).all()

    class Cached:                       # a dataset whose dimensions are in the cache is not clustered again
        name, voxel_size = "SemanticKITTIDataset", 0.05

        def __len__(self):
            raise AssertionError("the cache was not used")

    np.save(str(tmp_path / "semantickittidataset.npy"), s)
    cached = data.scaling_params([Cached()], [t], cache_dir=str(tmp_path))
    assert cached[0].tobytes() == data.scaling_params([s], [t])[0].tobytes()


def test_recorded_scaling_has_the_reference_layout():
    for k, c in enumerate(META["scaling"]):
        a = G12[f"p{k}_scaling"]
        assert a.dtype == np.float32 and a.shape == (len(c["sources"]), len(c["targets"]), 3)
    assert (G12["p0_scaling"] > 1).all()              # nuScenes-like cars are larger: scaling towards them spreads voxels


@pytest.mark.parametrize("k", range(len(META["items"])))
def test_item_draws_replay(k):
    it = META["items"][k]
    scaling = sn_ref.item_scaling(G12, it["kind"], it["which"])
    rng = np.random.RandomState(it["seed"])
    rows = data.draw_scaling(rng, scaling, len(it["scans"]))
    if it["kind"] == "single":
        assert it["draws"] == [] and rows[0].tobytes() == scaling[0][0].tobytes()
        two_targets = [np.stack([scaling[0][0], scaling[0][0] * 2])]      # one source, two targets: still the first row
        assert data.draw_scaling(rng, two_targets, 1)[0].tobytes() == scaling[0][0].tobytes()
    else:
        assert [r.tobytes() for r in rows] == [scaling[s][d].tobytes() for s, d in enumerate(it["draws"])]


# ------------------------------------------------------------------ the synthetic car scans
def test_old_configurations_are_unchanged_and_cars_are_class_zero():
    for cfg in ("kitti120k", "source8k"):
        vox, _ = synth.scan_voxels(0, cfg)
        assert synth.stride_counts(vox) == synth.BASELINE_COUNTS[cfg], cfg
    vox, _ = synth.mix3d_voxels(0)
    assert synth.stride_counts(vox) == synth.BASELINE_COUNTS["nusc35k+mix3d"]
    vox, labels = synth.scan_voxels(0, "highres524k")
    assert synth.stride_counts(vox) == synth.BASELINE_COUNTS["highres524k"]
    assert set(np.unique(labels).tolist()) == set(range(-1, 7))
    for cfg in ("kitti120k_cars", "nusc35k_cars"):
        vox, labels = synth.scan_voxels(2, cfg)
        assert np.unique(vox, axis=0).shape[0] == vox.shape[0]
        assert set(np.unique(labels).tolist()) == set(range(-1, 7)) and (labels == 0).sum() > 2000
        car = vox[labels == 0].astype(np.float64) * synth.CONFIGS[cfg]["voxel"]
        h = synth.CONFIGS[cfg]["h"]
        assert car[:, 2].min() > -h - 0.2 and car[:, 2].max() < -h + 1.8 * synth.CONFIGS[cfg]["cars"] + 0.2
        d = np.hypot(car[:, 0], car[:, 1])
        assert d.min() > 1.5 and d.max() < 14 + 3.5
    assert synth.car_boxes(3, 1.1)[:, 2:] == pytest.approx(synth.car_boxes(3, 1.0)[:, 2:] * 1.1)
    assert SynthDataset(4, "nusc35k_cars").name == "NuScenesDataset" and SynthDataset(4, "kitti120k").name == "kitti120k"


# ------------------------------------------------------------------ the scaled dataset
def _recording(ds, log):
    def scale(scan, row, voxel_size):
        log.append((int(scan["coordinates"].shape[0]), np.asarray(row).tobytes()))
        return {"coordinates": scan["coordinates"], "features": scan["features"], "sem_labels": scan["sem_labels"]}
    ds.scale = scale


SCALING2 = [np.array([[1.1, 1.2, 1.3], [0.9, 0.8, 0.7], [1.0, 1.5, 0.5]], np.float32),
            np.array([[2.0, 2.0, 2.0], [0.5, 0.5, 0.5], [1.0, 1.0, 1.0]], np.float32)]


@pytest.mark.parametrize("sources", [1, 2])
def test_scaled_items_do_not_depend_on_the_batching(sources):
    configs = ("source8k", "source8k")[:sources]
    make = lambda: ScaledSynthScans(4, configs, ("nusc35k", "kitti120k", "source8k"), seed=7, scaling=SCALING2[:sources])
    ds = make()
    whole, split = [], []
    _recording(ds, whole)
    ds.set_epoch(1)
    b = ds.batch([0, 1, 2, 3], "cpu")
    _recording(ds, split)
    for part in ([2], [0, 3], [1]):
        ds.batch(part, "cpu")
    order = {i: k for k, i in enumerate([2, 0, 3, 1])}
    assert [split[sources * order[i] + s] for i in range(4) for s in range(sources)] == whole
    assert b["coords_int"].dtype == torch.int32 and b["coords_int"][:, 0].unique().tolist() == [0, 1, 2, 3]
    keys = {"coords_int", "source_coordinates0", "source_features0", "source_sem_labels0"}
    if sources == 2:
        keys |= {"coords_int1", "source_coordinates1", "source_features1", "source_sem_labels1"}
        assert len({w[1] for w in whole[0::2]}) > 1           # the target row is drawn per item
        again = []
        _recording(ds, again)
        ds.set_epoch(2)
        ds.batch([0, 1, 2, 3], "cpu")
        assert [a[1] for a in again] != [w[1] for w in whole]
    else:
        assert {w[1] for w in whole} == {SCALING2[0][0].tobytes()}       # one source: always the first target's row
    assert set(b) == keys and ds.num_sources == sources and len(ds) == 4
    resumed = []
    ds2 = make()
    _recording(ds2, resumed)
    ds2.set_epoch(1)
    ds2.batch([0, 1, 2, 3], "cpu")
    assert resumed == whole


def test_scaled_dataset_refusals():
    with pytest.raises(NotImplementedError):
        ScaledSynthScans(2, ("source8k",) * 3, ("nusc35k",), scaling=SCALING2 + SCALING2[:1])
    with pytest.raises(ValueError):
        ScaledSynthScans(2, ("source8k",), (), scaling=SCALING2[:1])
    with pytest.raises(ValueError):
        ScaledSynthScans(2, ("source8k", "source8k"), ("nusc35k",), scaling=SCALING2[:1])


# ------------------------------------------------------------------ command line
def test_cli_sn_targets():
    a = parse_args(["--model", "MinkUNet34", "--config", "kitti120k_cars", "--sn-targets", "nusc35k_cars"])
    assert a.sn_targets == ["nusc35k_cars"] and a.sources is None and a.mix is None
    b = parse_args(["--model", "MinkUNet34IBN", "--sources", "kitti120k_cars", "nusc35k_cars", "--sn-targets",
                    "nusc35k_cars", "kitti120k_cars", "--lr", "0.01", "--scheduler", "ExponentialLR"])
    assert b.sn_targets == ["nusc35k_cars", "kitti120k_cars"] and b.sources == ["kitti120k_cars", "nusc35k_cars"]
    assert parse_args([]).sn_targets is None


@pytest.mark.parametrize("argv", [["--sn-targets", "nusc35k_cars"],
                                  ["--model", "MinkUNet34BEV", "--sn-targets", "nusc35k_cars"],
                                  ["--model", "MinkUNet34Robust", "--sn-targets", "nusc35k_cars"],
                                  ["--model", "MinkUNet34", "--sn-targets", "nusc35k_cars", "--mix", "cosmix"],
                                  ["--model", "MinkUNet34", "--sn-targets", "nusc35k_cars", "--mix3d"],
                                  ["--model", "MinkUNet34", "--sn-targets", "no_such_config"],
                                  ["--model", "MinkUNet34", "--sn-targets"]])
def test_cli_sn_refusals(argv, capsys):
    with pytest.raises(SystemExit):
        parse_args(argv)


# ------------------------------------------------------------------ C ABI and imports
def test_sn_symbols_are_declared_bound_and_exported():
    from lidog_amd import _lib, build
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    lib = __import__("ctypes").CDLL(build.build())
    for name in SN_SYMBOLS:
        assert re.search(rf"\b{name}\(", header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert "cluster.hip" in build.SOURCES
    assert _lib.ABI_VERSION == 9 and lib.lidog_abi_version() == 9
    assert _lib._RESTYPES["lidog_dbscan_ws"] is _lib._i64


def test_cluster_refuses_cpu_tensors_and_bad_arguments():
    from lidog_amd import cluster
    c = torch.zeros((12, 3), dtype=torch.int32)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        cluster.dbscan(c, 0.05)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        cluster.cluster_boxes(c, torch.zeros(12, dtype=torch.int32))
    scan = {"coordinates": c, "features": torch.ones((12, 1)), "sem_labels": torch.zeros(12, dtype=torch.int64)}
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        data.sn_scale(scan, [1.0, 1.0, 1.0])


def test_the_package_imports_neither_sklearn_nor_the_oracle():
    code = ("import sys, lidog_amd, lidog_amd.cluster, lidog_amd.data, lidog_amd.train\n"
            "bad = [m for m in sys.modules if m.split('.')[0] in ('sklearn', 'oracle', 'scipy')]\n"
            "assert not bad, bad\n")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO, timeout=300)
