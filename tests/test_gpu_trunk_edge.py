"""Trunk executor (csrc/trunk.hip, lidog_amd/trunk.py) against the operator path (lidog_amd/me.py), byte for byte, on the
batches a LiDAR-shaped scene never shows: the edge scenes of tests/sconv_ref.py taken through whole optimiser steps --
levels of one or two rows (BatchNorm over a count of 1 in every place that finishes statistics), 127 / 128 / 129 rows at
the 128-row tile edge, maps with centre pairs only, a one-voxel scan next to a full one, a scan without voxels, batch
index 4095 with coordinates at the ends of the key range -- then one model stepped on a large, a one-voxel, a 129-voxel
and the large batch again (the arenas the executor keeps per model shrink and grow), and an empty input.

The per-layer kernels are held to float64 on these same scenes (test_gpu_sconv_edge64.py, test_gpu_bn_rows64.py,
test_gpu_sconv_wgrad64.py); here the executor's own code is: arena planning from rows * channels, ReLU bit masks,
the BatchNorm + ReLU fold into the next convolution's staging, BatchNorm-backward statistics in the data-gradient
epilogue, row-list vs output-stationary form per map, cat / split / add on arena addresses.

Everything is compared as BYTES: a level of one row may legitimately give the same non-finite pattern on both paths,
and a NaN must not make an equal pair look unequal.  tests/test_trunk_cpu.py pins the row counts per level the cases
rely on.

Outcome when written: the executor took every listed batch, every case is byte-identical, and nothing compared is
non-finite in any case, the one- and two-row scenes included (recorded property `non_finite`).  An empty input raises
RuntimeError("... bn_stats: finalising needs the row count") on the operator path, with the executor on and off alike.

Wall time (MI355X, one pytest run of this file and test_gpu_trunk.py, --durations=0): this file 22.9 s over 38 cases,
0.33 to 0.95 s each and 1.49 s for the first (it loads the library and draws the seeded weights); test_gpu_trunk.py
25.3 s over 23 cases, its step cases 0.85 to 1.17 s, its slowest (two data-parallel ranks) 4.09 s.
"""
import numpy as np
import pytest
import torch

import sconv_ref as R
from helpers import seeded_state_dict
from test_gpu_trunk import _buffers, _grads

pytestmark = pytest.mark.gpu

TAKEN = "_TrunkFnBackward"
BEV_SCENES = ("tiny_1", "tiny_2", "tiny_127", "tiny_128", "tiny_129", "line_x129", "isolated", "checkerboard",
              "dense_cube_odd", "one_and_many")
# levels of one or two rows (tiny_*), batch statistics of two rows at +-65535 (range_ends): equality only
MAY_BE_NON_FINITE = ("tiny_1", "tiny_2", "range_ends")
SETTINGS = {"fused": (7, 1), "plain_sequence": (0, 1), "fused_output_stationary": (7, 2)}
CASES = [(s, k, True) for s in BEV_SCENES + ("range_ends",) for k in SETTINGS] + \
        [(s, "fused", False) for s in ("tiny_1", "tiny_129", "isolated")]

_SEEDS = {}
_REFERENCE = {}     # the operator path's run of the last (scene, os_mode, overlap): the fusions are the executor's alone


@pytest.fixture(scope="module", autouse=True)
def _release_shared_results():
    yield
    _SEEDS.clear()
    _REFERENCE.clear()


def _seeded(model, seed):
    """helpers.seeded_state_dict, drawn once per model class and seed (it walks 155 MB on the host)"""
    key = (type(model).__name__, seed)
    if key not in _SEEDS:
        _SEEDS[key] = seeded_state_dict(model, seed)
    return _SEEDS[key]


def _model(kind="MinkUNet34BEV", seed=5):
    import lidog_amd
    if kind == "MinkUNet34BEV":
        m = lidog_amd.MinkUNet34BEV(1, 7, 3, mapping_bound_2d=5.0).cuda()
    else:
        m = lidog_amd.MinkUNet34(1, 7, 3).cuda()
    m.load_state_dict(_seeded(m, seed))
    return m.train()


def _batch(name, seed=61, bev=17):
    """the step's batch of a scene: coordinates as they are, seeded normal features (rows in symmetric positions of a
    scene must not be equal), seeded labels in [-1, 7)"""
    c = R.scene(name)
    n, B = c.shape[0], int(c[:, 0].max()) + 1
    g = torch.Generator().manual_seed(seed)
    coords = torch.from_numpy(c).cuda()
    return {"coords_int": coords, "source_coordinates0": coords.float(),
            "source_features0": torch.randn((n, 1), generator=g).cuda(),
            "source_sem_labels0": torch.randint(-1, 7, (n,), generator=g).cuda(),
            "source_bev_labels0": {"block8": torch.randint(-1, 7, (B, bev, bev), generator=g).cuda()}}


def _bytes(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


def _same_bytes(a, b, what, diffs):
    """appends to `diffs` one line per entry of the dictionaries a / b (tensors or None) whose bytes differ"""
    assert a.keys() == b.keys(), what
    for k in a:
        if a[k] is None or b[k] is None:
            if not (a[k] is None and b[k] is None):
                diffs.append(f"{what} {k}: one side has none")
        elif a[k].shape != b[k].shape or a[k].dtype != b[k].dtype:
            diffs.append(f"{what} {k}: {tuple(a[k].shape)} {a[k].dtype} vs {tuple(b[k].shape)} {b[k].dtype}")
        elif _bytes(a[k]) != _bytes(b[k]):
            x, y = a[k].double(), b[k].double()
            ne = a[k].contiguous().view(-1).view(torch.uint8) != b[k].contiguous().view(-1).view(torch.uint8)
            diffs.append(f"{what} {k}: {int(ne.sum())} bytes differ, max |diff| {float((x - y).abs().nan_to_num().max()):.3e}")


def _non_finite(named):
    return sorted(k for k, t in named.items() if t is not None and t.is_floating_point() and not bool(torch.isfinite(t).all()))


class _Watch:
    """which maps took the output-stationary form: on the operator path me._os_rows hands the sorted rows to the
    convolution that then launches csrc/sconv_os.hip; the executor gets them as table columns (TM_PERM and the two
    behind it) and, for such a map, NO per-row lists -- so its C walk can only launch the output-stationary kernels there
    (trunk.hip refuses a 3^3 map with neither)"""

    def __init__(self, monkeypatch):
        from lidog_amd import me as ME, trunk
        self.os_maps = set()           # (rows, pairs) of every map that ran output-stationary
        self.declined = 0
        os_rows, build = ME._os_rows, trunk._build_tables

        def watched_os_rows(m, swap, Cin, Cout):
            got = os_rows(m, swap, Cin, Cout)
            if got is not None:
                self.os_maps.add((m.n_out, m.P))
            return got

        def watched_build(prog, x, run):
            got = build(prog, x, run)
            if got is None:
                self.declined += 1
                return got
            for row, ok in zip(run.maps, prog.os_ok):
                if row[14] and row[15] and row[16] and ok:        # TM_PERM, TM_WMASK, TM_ORDER
                    assert row[0] == 27 and not row[6:10].any(), "sorted rows AND row lists: which form ran is open"
                    self.os_maps.add((int(row[2]), int(row[3])))
            return got

        monkeypatch.setattr(ME, "_os_rows", watched_os_rows)
        monkeypatch.setattr(trunk, "_build_tables", watched_build)


def _run_steps(step_cls, kind, batches, on, watch, pre=None):
    """one model, one optimiser (Adam on flat buffers), one step per batch; everything that is compared"""
    from lidog_amd import trunk
    from lidog_amd.optim import make_optimizer
    trunk.set_enabled(on)
    watch.os_maps, watch.declined = set(), 0
    model = _model(kind)
    step = step_cls(model, make_optimizer("Adam", model, 1e-2, weight_decay=1e-4))
    if pre is not None:
        pre(model)
        watch.declined = 0
    seen = []
    hook = model.register_forward_hook(lambda mod, args, out: seen.append((out[0] if isinstance(out, tuple) else out).F.detach().clone()))
    res = {"losses": [], "logits": {}, "grads": None, "os_maps": None}
    try:
        for it, batch in enumerate(batches):
            out = step.training_step(batch)
            assert (step.last_path == TAKEN) == on, f"step {it}: the pass went through {step.last_path}"
            res["losses"].append({k: v.clone() for k, v in out.items()})
            res["logits"][f"step{it}"] = seen.pop()
            if it == 0:
                res["grads"] = _grads(model)
    finally:
        hook.remove()
    torch.cuda.synchronize()
    assert watch.declined == 0, "the executor declined a batch of the table"
    res["state"] = _buffers(model)
    res["os_maps"] = set(watch.os_maps)
    return res


def _compare(got, want, finite, record_property):
    diffs = []
    for it, (a, b) in enumerate(zip(got["losses"], want["losses"])):
        _same_bytes(a, b, f"step {it}", diffs)
    _same_bytes(got["logits"], want["logits"], "logits", diffs)
    _same_bytes(got["grads"], want["grads"], "gradient after step 0", diffs)
    _same_bytes(got["state"], want["state"], "state after the last step", diffs)
    everything = {**{f"loss{it}.{k}": v for it, d in enumerate(got["losses"]) for k, v in d.items()},
                  **{f"logits.{k}": v for k, v in got["logits"].items()},
                  **{f"grad.{k}": v for k, v in got["grads"].items()}, **{f"state.{k}": v for k, v in got["state"].items()}}
    bad = _non_finite(everything)
    print(f"non-finite tensors (executor): {len(bad)} of {len(everything)}: {bad[:12]}{' ...' if len(bad) > 12 else ''}")
    record_property("non_finite", bad)
    assert not diffs, f"{len(diffs)} entries differ between executor and operator path:\n" + "\n".join(diffs[:20])
    if finite:
        assert not bad, f"non-finite: {bad[:20]}"
    return bad


@pytest.mark.parametrize("scene,setting,overlap", CASES,
                         ids=[f"{s}-{k}{'' if ov else '-weight_gradients_in_line'}" for s, k, ov in CASES])
def test_edge_batch_steps_are_byte_identical_to_the_operator_path(scene, setting, overlap, monkeypatch, record_property):
    """2 optimiser steps (the same batch twice, Adam on flat buffers) of the LiDOG step on MinkUNet34BEV -- for
    range_ends (batch indices 0 and 4095: a [4096, 17, 17] label image is not its point) of the source step on
    MinkUNet34 -- executor on vs off: the losses of both steps, the logits of both, every parameter gradient of step 0,
    every entry of the state_dict after step 1.  os_mode 2 sends every symmetric 3^3 map (all five levels here, from 1
    row up: KernelMap.sorted returns rows for every one of them) through csrc/sconv_os.hip on both paths.
    The operator path's run does not depend on the executor's fusions: it is computed once per (scene, os_mode, overlap)
    and shared by the cases that follow each other."""
    from lidog_amd import me as ME, trunk
    from lidog_amd.trainer import LiDOGStep, SourceStep
    fusions, os_mode = SETTINGS[setting]
    monkeypatch.setattr(ME, "_SCONV_OS", os_mode)
    monkeypatch.setattr(ME, "_OS_HINT", {})     # which maps the previous batch sorted: not this case's business
    watch = _Watch(monkeypatch)
    ME.set_backward_overlap(overlap)
    before = trunk.set_fusions(fusions)
    try:
        step_cls, kind = (SourceStep, "MinkUNet34") if scene == "range_ends" else (LiDOGStep, "MinkUNet34BEV")
        batches = [_batch(scene)] * 2
        key = (scene, os_mode, overlap)
        if key not in _REFERENCE:
            _REFERENCE.clear()
            _REFERENCE[key] = _run_steps(step_cls, kind, batches, False, watch)
        want = _REFERENCE[key]
        got = _run_steps(step_cls, kind, batches, True, watch)
    finally:
        trunk.set_enabled(True)
        trunk.set_fusions(before)
        ME.set_backward_overlap(True)
    _compare(got, want, scene not in MAY_BE_NON_FINITE, record_property)
    trunk_grads = {k: v for k, v in got["grads"].items() if not k.startswith("encoders2d")}
    assert any(v is not None and bool((v != 0).any()) for v in trunk_grads.values()), "no trunk gradient moved"
    assert _bytes(got["losses"][0]["loss"]) != _bytes(got["losses"][1]["loss"]), "step 1 lost what step 0 lost"
    if os_mode == 2:
        levels = {R.strided(R.scene(scene), 2 ** lv).shape[0] for lv in range(5)}
        assert got["os_maps"] == want["os_maps"], (got["os_maps"], want["os_maps"])
        assert {n for n, _ in got["os_maps"]} == levels, f"output-stationary on {got['os_maps']}, levels of {levels} rows"
    else:
        assert not got["os_maps"] and not want["os_maps"]


def test_arenas_kept_across_batch_sizes():
    """One model, one optimiser, four steps: twin_scans (4044 rows), tiny_1, tiny_129, twin_scans.  The executor keeps
    its activation, gradient and scratch arenas per model (trunk._Arenas): the small steps run in memory full of the
    large batch's values (a read past a buffer's rows sees plausible numbers there, not zeros), the last one grows them
    again.  Losses, logits of every step and the final state_dict, byte for byte, against the operator path.
    Then the same on a fresh model that first saw one forward pass on twin_scans under no_grad, which the executor
    declines: that pass moves the running statistics and the batch counters (training mode; asserted), so the seeded
    state is loaded again behind it -- in place, the parameters stay in the optimiser's flat buffers -- and the four
    steps must give the bytes of the first executor run."""
    import lidog_amd.me as ME
    from lidog_amd import trunk
    from lidog_amd.trainer import LiDOGStep

    class _NoWatch:
        os_maps, declined = set(), 0

    def declined_pass(model):
        b = _batch("twin_scans")
        with torch.no_grad():
            sem, _ = model(ME.SparseTensor(coordinates=b["coords_int"], features=b["source_features0"]), is_train=True)
        assert sem.F.grad_fn is None
        moved = [int(v) for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")]
        assert moved and all(v == 1 for v in moved)
        model.load_state_dict(_seeded(model, 5))
        assert model.training

    batches = [_batch(name, seed) for name, seed in (("twin_scans", 61), ("tiny_1", 62), ("tiny_129", 63), ("twin_scans", 64))]
    try:
        want = _run_steps(LiDOGStep, "MinkUNet34BEV", batches, False, _NoWatch())
        got = _run_steps(LiDOGStep, "MinkUNet34BEV", batches, True, _NoWatch())
        again = _run_steps(LiDOGStep, "MinkUNet34BEV", batches, True, _NoWatch(), pre=declined_pass)
    finally:
        trunk.set_enabled(True)
    for a, b, what in ((got, want, "executor vs operator path"), (again, got, "behind a declined pass vs without")):
        diffs = []
        for it, (x, y) in enumerate(zip(a["losses"], b["losses"])):
            _same_bytes(x, y, f"step {it}", diffs)
        _same_bytes(a["logits"], b["logits"], "logits", diffs)
        _same_bytes(a["state"], b["state"], "final state", diffs)
        assert not diffs, f"{what}: {len(diffs)} entries differ:\n" + "\n".join(diffs[:20])


def test_an_empty_input_is_declined_and_behaves_as_on_the_operator_path(record_property):
    """[0, 4] coordinates in training mode: no level has a row, so trunk._build_tables declines before it moves a
    BatchNorm batch counter.  Whatever the operator path does with such a batch (its output, or the exception it raises)
    the model must do with the executor on as well, and the counters must stand where the operator path alone leaves
    them."""
    import lidog_amd.me as ME
    from lidog_amd import trunk
    coords = torch.zeros((0, 4), dtype=torch.int32, device="cuda")
    feats = torch.zeros((0, 1), device="cuda")
    res = {}
    try:
        for on in (False, True):
            trunk.set_enabled(on)
            model = _model()
            try:
                sem, bev = model(ME.SparseTensor(coordinates=coords, features=feats), is_train=True)
                assert type(sem.F.grad_fn).__name__ != TAKEN
                what = ("output", {"logits": sem.F.detach().clone(), **{k: v.detach().clone() for k, v in bev.items()}})
            except AssertionError:
                raise
            except Exception as e:      # noqa: BLE001 -- whatever the operator path raises is the yardstick
                what = ("raised", type(e), str(e))
            torch.cuda.synchronize()
            counters = {k: v.clone() for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")}
            res[on] = (what, counters)
    finally:
        trunk.set_enabled(True)
    (want, want_counters), (got, got_counters) = res[False], res[True]
    if want[0] == "raised":
        print(f"operator path on an empty input raises {want[1].__name__}: {want[2]}")
        record_property("operator_path", f"{want[1].__name__}: {want[2]}")
        assert got[0] == "raised" and got[1] is want[1], (got, want)
    else:
        print(f"operator path on an empty input returns { {k: tuple(v.shape) for k, v in want[1].items()} }")
        record_property("operator_path", "output")
        assert got[0] == "output", got
        diffs = []
        _same_bytes(got[1], want[1], "output", diffs)
        assert not diffs, diffs
    # the counters: what the operator path alone leaves (a pass that ran moved each at most once), nothing on top of it
    diffs = []
    _same_bytes(got_counters, want_counters, "counter", diffs)
    assert not diffs, diffs
    assert all(int(v) <= 1 for v in got_counters.values())
