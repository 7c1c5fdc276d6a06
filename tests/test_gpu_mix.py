"""PointCutMix / CoSMix on the GPU: both merges equal the reference's merge_data bit for bit on every G11 case, the
split kernel equals a stable argsort, the histogram equals np.bincount, and a two-epoch --mix fit validates, saves and
resumes."""
import functools
import os

import numpy as np
import pytest
import torch

import mix_ref
from lidog_amd import _lib, data
from lidog_amd._lib import call, ptr
from lidog_amd.data import cosmix_merge, pointcutmix_merge

pytestmark = pytest.mark.gpu

G11 = mix_ref.load_g11()


@functools.lru_cache(maxsize=None)
def _host_scans(config0, scan0, config1, scan1, one_class, limit):
    c = dict(config0=config0, scan0=scan0, config1=config1, scan1=scan1, one_class=one_class, limit=limit)
    return mix_ref.case_scans(c)


def _device(scan):
    d = {k: torch.from_numpy(np.asarray(v)).cuda() for k, v in scan.items() if k != "idx"}
    d["idx"] = torch.tensor(int(scan["idx"]))
    return d


def _ids(cases):
    return [f"{c['method']}-{c['config0']}-{c['config1']}-seed{c['seed']}{'-raises' if c['outcome'] == 'raises' else ''}"
            for c, _ in cases]


@pytest.mark.parametrize("case", G11, ids=_ids(G11))
def test_merge_equals_the_reference(case):
    c, arr = case
    s0, s1 = (_device(s) for s in _host_scans(c["config0"], c["scan0"], c["config1"], c["scan1"], c["one_class"],
                                                c["limit"]))
    voxel = mix_ref.voxel_size(c)
    if c["method"] == "pointcutmix":
        merge = functools.partial(pointcutmix_merge, voxel_size=voxel)
    else:
        merge = functools.partial(cosmix_merge, voxel_size=voxel, class_weights=(arr["w0"], arr["w1"]),
                                  sub_p=c["sub_p"])
    np.random.seed(c["seed"])
    if c["outcome"] == "raises":
        with pytest.raises(ValueError):
            merge(s0, s1, rng=np.random)
        return
    out = merge(s0, s1, rng=np.random)
    assert out["source"] == c["source"]
    assert out["idx"].tolist() == c["idx"]
    got = {k: out[k].cpu().numpy() for k, _ in mix_ref.OUTPUTS}
    assert got["coordinates"].dtype == np.int32 and got["index"].dtype == np.int64
    for k, dt in mix_ref.OUTPUTS:
        a = got[k].astype(dt)
        assert a.shape[0] == c["rows"], k
        if k in arr:
            np.testing.assert_array_equal(a, arr[k], err_msg=k)
        assert mix_ref.digest(a) == c["digests"][k], k


def test_merge_refuses_cpu_tensors():
    s = {"coordinates": torch.zeros((4, 3), dtype=torch.int32), "features": torch.ones((4, 1)),
         "sem_labels": torch.zeros(4, dtype=torch.int64)}
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        pointcutmix_merge(s, s)
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        cosmix_merge(s, s, class_weights=(np.ones(7), np.ones(7)))


# ------------------------------------------------------------------ kernels
def _split(keys, table, S):
    k = torch.from_numpy(keys.astype(np.int32)).cuda()
    t = torch.from_numpy(table.astype(np.int32)).cuda()
    n = keys.shape[0]
    rows = torch.full((max(n, 1),), -7, dtype=torch.int32, device="cuda")
    start = torch.full((S + 1,), -7, dtype=torch.int32, device="cuda")
    ws = torch.empty(_lib.load().lidog_mix_split_ws(n, S), dtype=torch.int32, device="cuda")
    call("lidog_mix_split", ptr(k), n, ptr(t), t.shape[0], S, ptr(rows), ptr(start), ptr(ws))
    start = start.cpu().numpy()
    return rows.cpu().numpy()[:start[-1]], start


def _expected(keys, table, S):
    inr = (keys >= 0) & (keys < table.shape[0])
    slot = np.where(inr, table[np.clip(keys, 0, table.shape[0] - 1)], -1)
    slot = np.where((slot >= 0) & (slot < S), slot, -1)
    taken = np.nonzero(slot >= 0)[0]
    order = taken[np.argsort(slot[taken], kind="stable")]
    start = np.concatenate([[0], np.cumsum(np.bincount(slot[taken], minlength=S))])
    return order, start


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100003])
@pytest.mark.parametrize("S", [1, 4, 9, 32])
def test_split_equals_a_stable_argsort(n, S):
    rng = np.random.default_rng(n * 100 + S)
    nkeys = 3 * S + 5
    table = rng.integers(-1, S, nkeys)
    if S > 1:
        table[table == S - 1] = -1                                         # an empty slot
    keys = rng.integers(-3, nkeys + 3, n)
    cases = [(keys, table), (rng.integers(0, 2, n), np.array([0, 0])),                 # one slot holds everything
             (keys, np.full(nkeys, -1))]                                                # nothing selected
    for keys_, table_ in cases:
        order, start = _expected(keys_, table_, S)
        got, gstart = _split(keys_, table_, S)
        np.testing.assert_array_equal(gstart, start)
        np.testing.assert_array_equal(got, order)
        again, _ = _split(keys_, table_, S)
        np.testing.assert_array_equal(again, got)


def test_split_many_slots_and_rows():
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 256, 1 << 20)
    table = rng.permutation(256) - 16         # 240 slots, 16 keys not taken
    order, start = _expected(keys, table, 240)
    got, gstart = _split(keys, table, 240)
    np.testing.assert_array_equal(gstart, start)
    np.testing.assert_array_equal(got, order)


@pytest.mark.parametrize("n", [0, 1, 100003])
@pytest.mark.parametrize("nbins", [1, 7, 130, 5000])
def test_histogram_equals_bincount(n, nbins):
    keys = np.random.default_rng(n + nbins).integers(-5, nbins + 5, n).astype(np.int32)
    k = torch.from_numpy(keys).cuda()
    counts = torch.full((nbins,), 123, dtype=torch.int32, device="cuda")
    call("lidog_mix_histogram", ptr(k), n, nbins, ptr(counts))
    inr = keys[(keys >= 0) & (keys < nbins)]
    np.testing.assert_array_equal(counts.cpu().numpy(), np.bincount(inr, minlength=nbins))


def test_merge_on_a_busy_stream_hands_over_an_equal_result():
    """called from another stream than the merge stream (a training step queued there), the result is the same"""
    c, arr = next(x for x in G11 if x[0]["method"] == "cosmix" and x[0]["config0"] == "nusc35k")
    s0, s1 = (_device(s) for s in _host_scans(c["config0"], c["scan0"], c["config1"], c["scan1"], c["one_class"],
                                                c["limit"]))
    kw = dict(voxel_size=mix_ref.voxel_size(c), class_weights=(arr["w0"], arr["w1"]), sub_p=c["sub_p"])
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        a = torch.randn(2048, 2048, device="cuda")
        for _ in range(4):
            a = a @ a
            a = a / a.norm()
        out = cosmix_merge(s0, s1, rng=np.random.RandomState(c["seed"]), **kw)
        feats = out["features"] + 0.0
    torch.cuda.synchronize()
    assert mix_ref.digest(feats.cpu().numpy()) == c["digests"]["features"]
    assert data.merge_stream("cuda") != other


# ------------------------------------------------------------------ training
@pytest.mark.timeout(300)
@pytest.mark.parametrize("method,config", [("cosmix", "source8k"), ("pointcutmix", "nusc35k")])
def test_cli_mix_fit_validate_resume(method, config, tmp_path):
    from lidog_amd.train import MixedSynthScans, _fit_from_args, parse_args
    from lidog_amd.trainer import SourceStep
    argv = ["--model", "MinkUNet34", "--mix", method, "--config", config, "--epochs", "2", "--scans", "2", "--batch",
            "1", "--val-scans", "1", "--check-val-every-n-epoch", "1", "--save-dir", str(tmp_path)]
    fit = _fit_from_args(parse_args(argv))
    fit.log = lambda *_: None
    assert isinstance(fit.train_data, MixedSynthScans) and type(fit.step) is SourceStep and fit.step.num_sources == 1
    hist = fit.run()
    assert len(hist) == 2 and all(np.isfinite(h["losses"]).all() for h in hist)
    assert fit.train_data.epoch == 1
    for h in hist:
        assert set(h["validation"]) == {f"{config}:0", f"{config}:1"}
        assert all(np.isfinite(v["sem_loss"]) for v in h["validation"].values())
    assert os.path.exists(hist[1]["checkpoint"])
    again = _fit_from_args(parse_args(argv[:-1] + [str(tmp_path), "--auto-resume"]))
    assert again.epoch == 2 and again.global_step == fit.global_step
