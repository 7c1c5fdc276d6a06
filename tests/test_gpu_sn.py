"""The SN car-size scaling baseline on the GPU: cluster.dbscan equals sklearn's DBSCAN label for label on every G12 case
(integers: no tolerance), cluster_boxes the recorded boxes, average_dims / scaling_params the reference's float32 values
bit for bit, sn_scale every recorded item bit for bit, and `--sn-targets` trains, checkpoints and resumes."""
import functools

import numpy as np
import pytest
import torch

import sn_ref
from lidog_amd import cluster, data, synth

pytestmark = pytest.mark.gpu

META, G12 = sn_ref.load_g12()
VOXEL = META["voxel"]
LATTICE = sn_ref.lattice_cases(G12)


def _dbscan(coords):
    c = torch.from_numpy(np.ascontiguousarray(coords, dtype=np.int32)).cuda()
    labels, k = cluster.dbscan_count(c, VOXEL, eps=META["eps"], min_samples=META["min_samples"])
    assert labels.dtype == torch.int32 and labels.shape == (c.shape[0],)
    again = cluster.dbscan(c, VOXEL, eps=META["eps"], min_samples=META["min_samples"])
    assert labels.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()          # the same bytes on every run
    return c, labels, k


# ------------------------------------------------------------------ labels
@pytest.mark.parametrize("k", range(len(LATTICE)),
                         ids=[f"seed{s}{'-sphere' if LATTICE[i][2] else ''}" for i, s in enumerate(META["lattice_seeds"])])
def test_dbscan_equals_sklearn_on_the_lattice_cases(k):
    coords, want, _ = LATTICE[k]
    _, labels, n_clusters = _dbscan(coords)
    np.testing.assert_array_equal(labels.cpu().numpy(), want)
    assert n_clusters == want.max() + 1


@pytest.mark.parametrize("name", META["edge"])
def test_dbscan_equals_sklearn_on_the_edge_cases(name):
    coords = sn_ref.edge_cases()[name]
    c, labels, n_clusters = _dbscan(coords)
    want = G12[f"edge_{name}_labels"].astype(np.int64)
    np.testing.assert_array_equal(labels.cpu().numpy(), want)
    assert n_clusters == want.max() + 1
    counts, lo, hi = cluster.cluster_boxes(c, labels)
    wc, wlo, whi = sn_ref.boxes_np(coords, want)
    np.testing.assert_array_equal(counts.cpu().numpy(), wc)
    np.testing.assert_array_equal(lo.cpu().numpy(), wlo)
    np.testing.assert_array_equal(hi.cpu().numpy(), whi)


CAR_SCANS = [(k, s) for k, r in enumerate(META["stats"]) for s in r["scans"] if s["clustered"]]


@pytest.mark.parametrize("case", CAR_SCANS,
                         ids=[f"{META['stats'][k]['dataset']}-seed{META['stats'][k]['seed']}-scan{s['scan']}" for k, s in CAR_SCANS])
def test_dbscan_and_boxes_equal_the_reference_on_the_car_scans(case):
    k, s = case
    car = sn_ref.car_voxels(META["stats"][k]["dataset"], s["scan"])
    assert car.shape[0] == s["car_voxels"]
    c, labels, n_clusters = _dbscan(car)
    got = labels.cpu().numpy()
    want = G12[f"s{k}_{s['slot']}_labels"]
    np.testing.assert_array_equal(got, want.astype(np.int32))
    assert sn_ref.digest(got.astype(np.int16)) == s["labels_sha1"] and n_clusters == s["clusters"]
    assert int((got == -1).sum()) == s["noise"]
    counts, lo, hi = cluster.cluster_boxes(c, labels, n_clusters)
    assert counts.dtype == torch.int64 and lo.dtype == torch.int32 and hi.dtype == torch.int32
    np.testing.assert_array_equal(counts.cpu().numpy(), G12[f"s{k}_{s['slot']}_counts"])
    np.testing.assert_array_equal(lo.cpu().numpy(), G12[f"s{k}_{s['slot']}_lo"])
    np.testing.assert_array_equal(hi.cpu().numpy(), G12[f"s{k}_{s['slot']}_hi"])
    again = cluster.cluster_boxes(c, labels)                  # k read from the labels; the same bytes
    assert all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(again, (counts, lo, hi)))


def test_dbscan_does_not_depend_on_the_row_order_of_its_graph():
    """a permuted input gives the same partition, renumbered by the smallest core row (checked against the restatement)"""
    coords, _, _ = LATTICE[0]
    perm = np.random.default_rng(0).permutation(len(coords))
    _, labels, _ = _dbscan(coords[perm])
    np.testing.assert_array_equal(labels.cpu().numpy(), sn_ref.dbscan_np(coords[perm]))


def test_dbscan_other_parameters_and_dtypes():
    coords, _, _ = LATTICE[1]
    for eps, ms, voxel in ((0.3, 4, 0.05), (0.5, 1, 0.05), (1.0, 10, 0.1), (0.26, 3, 0.02)):
        c = torch.from_numpy(coords).cuda().long()
        got = cluster.dbscan(c, voxel, eps=eps, min_samples=ms).cpu().numpy()
        np.testing.assert_array_equal(got, sn_ref.dbscan_np(coords, voxel, eps, ms), err_msg=str((eps, ms, voxel)))


def test_dbscan_empty_input_and_refusals():
    empty = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    labels, k = cluster.dbscan_count(empty, VOXEL)
    assert labels.shape == (0,) and labels.dtype == torch.int32 and k == 0
    counts, lo, hi = cluster.cluster_boxes(empty, labels)
    assert counts.shape == (0,) and lo.shape == (0, 3) and hi.shape == (0, 3)
    far = torch.tensor([[0, 0, 0], [65536, 0, 0]], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="65535"):
        cluster.dbscan(far, VOXEL)
    with pytest.raises(ValueError, match="65535"):
        cluster.dbscan(far.long() * 100000, VOXEL)
    corners = torch.tensor([[-65535] * 3, [65535] * 3], dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="2\\^32 cells"):           # 131071^3 cells of one voxel
        cluster.dbscan(corners, VOXEL, eps=0.05)
    ends = torch.tensor([[-65535, 0, 3], [65535, 0, 3]], dtype=torch.int32, device="cuda")      # the range's two ends
    np.testing.assert_array_equal(cluster.dbscan(ends, VOXEL, min_samples=1).cpu().numpy(), [0, 1])
    np.testing.assert_array_equal(cluster.dbscan(ends, VOXEL).cpu().numpy(), [-1, -1])
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        cluster.dbscan(corners.cpu(), VOXEL)
    with pytest.raises(ValueError):
        cluster.dbscan(corners, VOXEL, eps=0.0)


# ------------------------------------------------------------------ statistics
@pytest.mark.parametrize("k", range(len(META["stats"])), ids=[f"{r['dataset']}-seed{r['seed']}" for r in META["stats"]])
def test_average_dims_equals_the_reference(k):
    rec = META["stats"][k]
    ds = sn_ref.StubDataset(rec["dataset"])
    record = []
    np.random.seed(rec["seed"])
    if rec["outcome"] == "raises":
        with pytest.raises(ValueError):
            data.average_dims(ds, record=record)
    else:
        got = data.average_dims(ds, record=record)
        assert got.dtype == np.float32 and got.tobytes() == G12[f"s{k}_result"].tobytes()
        again = data.average_dims(sn_ref.StubDataset(rec["dataset"]), rng=np.random.RandomState(rec["seed"]))
        assert again.tobytes() == got.tobytes()
    assert ds.served == rec["drawn"]
    clustered = [s for s in rec["scans"] if s["clustered"]]
    assert [r[0] for r in record] == [s["scan"] for s in clustered]
    for (_, counts, lo, hi), s in zip(record, clustered):
        np.testing.assert_array_equal(counts, G12[f"s{k}_{s['slot']}_counts"])
        np.testing.assert_array_equal(lo, G12[f"s{k}_{s['slot']}_lo"])
        np.testing.assert_array_equal(hi, G12[f"s{k}_{s['slot']}_hi"])


@pytest.mark.parametrize("k", range(len(META["scaling"])),
                         ids=[f"{len(c['sources'])}x{len(c['targets'])}" for c in META["scaling"]])
def test_scaling_params_equal_the_reference(k, tmp_path):
    c = META["scaling"][k]
    np.random.seed(c["seed"])
    got = data.scaling_params([sn_ref.StubDataset(s) for s in c["sources"]], [sn_ref.StubDataset(t) for t in c["targets"]],
                              cache_dir=str(tmp_path))
    assert len(got) == len(c["sources"])
    assert np.stack(got).dtype == np.float32 and np.stack(got).tobytes() == G12[f"p{k}_scaling"].tobytes()


# ------------------------------------------------------------------ scaled items
def _device(scan):
    d = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in scan.items() if k != "idx"}
    d["idx"] = torch.tensor(int(scan["idx"]))
    return d


@pytest.mark.parametrize("k", range(len(META["items"])),
                         ids=[f"{it['kind']}-{it['scans'][0][0]}-{it['scans'][0][1]}" for it in META["items"]])
def test_sn_scale_equals_the_reference(k):
    it = META["items"][k]
    scaling = sn_ref.item_scaling(G12, it["kind"], it["which"])
    rows = data.draw_scaling(np.random.RandomState(it["seed"]), scaling, len(it["scans"]))
    for s, ((config, seed, limit), part) in enumerate(zip(it["scans"], it["parts"])):
        host = sn_ref.make_item_scan(config, seed, s, limit)
        out = data.sn_scale(_device(host), rows[s], voxel_size=VOXEL)
        assert out["coordinates"].dtype == torch.int32 and out["index"].dtype == torch.int64
        assert out["xyz"].shape[0] == part["rows_in"] and out["sampled_idx"].shape[0] == part["rows_in"]   # untouched
        for name, dt in sn_ref.OUTPUTS:
            a = out[name].cpu().numpy().astype(dt)
            assert a.shape[0] == part["rows"], name
            if part["full"]:
                np.testing.assert_array_equal(a, G12[f"i{k}_{s}_{name}"], err_msg=name)
            assert sn_ref.digest(a) == part["digests"][name], name


# ------------------------------------------------------------------ training
SEED = 1239


def _run(argv, tmp_path, sub):
    from lidog_amd.train import ScaledSynthScans, _fit_from_args, parse_args
    from lidog_amd.trainer import SourceStep
    fit = _fit_from_args(parse_args(argv + ["--save-dir", str(tmp_path / sub)]))
    fit.log = lambda *_: None
    assert isinstance(fit.train_data, ScaledSynthScans) and type(fit.step) is SourceStep
    seen = []
    own = fit.train_data.batch

    def batch(indices, device):
        b = own(indices, device)
        seen.append((fit.train_data.epoch, list(indices), b))
        return b

    fit.train_data.batch = batch
    return fit, seen


def _check_fit(argv, tmp_path, sources, targets):
    import os
    from lidog_amd.train import SynthDataset
    fit, seen = _run(argv + ["--epochs", "2"], tmp_path, "a")
    ds = fit.train_data
    assert fit.step.num_sources == len(sources) == ds.num_sources and fit.opt.lr == 0.01
    hist = fit.run()
    assert len(hist) == 2 and all(np.isfinite(h["losses"]).all() for h in hist) and ds.epoch == 1
    assert all(os.path.exists(h["checkpoint"]) for h in hist)
    assert hist[1]["lr"] == 0.01 * 0.99                                            # ExponentialLR(gamma=0.99), per epoch
    # the factors are those of the statistics over the same scans with the same draws
    n = len(ds)
    rng = np.random.RandomState(SEED)
    want = data.scaling_params([SynthDataset(n, c, s * synth.SOURCE1_SEED) for s, c in enumerate(sources)],
                               [SynthDataset(n, c, 10 ** 6 + t * synth.SOURCE1_SEED) for t, c in enumerate(targets)], rng=rng)
    assert np.stack(ds.scaling).tobytes() == np.stack(want).tobytes()
    assert all(a.shape == (len(targets), 3) for a in ds.scaling) and not (np.stack(want) == 1).all()
    # the first batch it trained on is sn_scale of the unscaled scans with those factors
    epoch, indices, b = seen[0]
    ds.set_epoch(epoch)
    for s in range(len(sources)):
        coords, labels = [], []
        for slot, i in enumerate(indices):
            src, j, row = ds.item(i)[s]
            if len(sources) == 1:
                assert j == i and row.tobytes() == want[0][0].tobytes()
            m = data.sn_scale(ds.scan(src, j, "cuda"), row, voxel_size=VOXEL)
            coords.append(torch.cat([torch.full((m["coordinates"].shape[0], 1), slot, dtype=torch.int32, device="cuda"),
                                     m["coordinates"]], dim=1))
            labels.append(m["sem_labels"])
        assert torch.equal(b["coords_int1" if s else "coords_int"], torch.cat(coords))
        assert torch.equal(b[f"source_sem_labels{s}"], torch.cat(labels))
        raw = sum(ds.scan(s, ds.item(i)[s][1], "cpu")["coordinates"].shape[0] for i in indices)
        assert 0 < b[f"source_features{s}"].shape[0] <= raw
    ds.set_epoch(1)
    # resumed from the epoch-0 checkpoint, the next step's loss is the same bit for bit
    again, _ = _run(argv + ["--epochs", "2", "--resume", hist[0]["checkpoint"]], tmp_path, "b")
    assert again.epoch == 1 and again.global_step == hist[0]["global_step"]
    assert np.stack(again.train_data.scaling).tobytes() == np.stack(ds.scaling).tobytes()
    h2 = again.run()
    print("epoch 1 losses:", hist[1]["losses"], "resumed:", h2[0]["losses"])
    assert len(h2) == 1 and h2[0]["epoch"] == 1
    assert np.float32(h2[0]["losses"][0]).tobytes() == np.float32(hist[1]["losses"][0]).tobytes()


# 20 % of 10 scans are 2 drawn scans per dataset: a run seed whose draws meet a car-shaped cluster in every dataset (as in
# the reference, statistics without one raise): SEED
COMMON = ["--model", "MinkUNet34", "--lr", "0.01", "--scheduler", "ExponentialLR", "--scans", "10", "--batch", "2",
          "--seed", str(SEED)]


@pytest.mark.timeout(600)
def test_cli_sn_one_source_trains_checkpoints_and_resumes(tmp_path):
    _check_fit(COMMON + ["--config", "kitti120k_cars", "--sn-targets", "nusc35k_cars"], tmp_path, ["kitti120k_cars"],
               ["nusc35k_cars"])


@pytest.mark.timeout(900)
def test_cli_sn_two_sources_train_checkpoint_and_resume(tmp_path):
    _check_fit(COMMON + ["--sources", "kitti120k_cars", "nusc35k_cars", "--sn-targets", "nusc35k_cars", "kitti120k_cars"],
               tmp_path, ["kitti120k_cars", "nusc35k_cars"], ["nusc35k_cars", "kitti120k_cars"])
