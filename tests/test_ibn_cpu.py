"""MinkUNet34IBN without a GPU: the IBN wiring of lidog_amd.minkunet bound to the CPU oracle (+ the instance-norm
restatement of tests/ibn_ref.py) reproduces G9 -- the reference class's logits; the product model's keys, shapes and
parameter count; the MinkowskiEngine alias; SyncBatchNorm conversion; the driver's --model choices; the C ABI."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import torch

from helpers import REPO, seeded_state_dict
from ibn_ref import G9, attach


def test_ibn_wiring_on_the_oracle_reproduces_g9_logits():
    import oracle.me_cpu as OME
    from lidog_amd.minkunet import make_models
    from oracle.ref_torch import Encoder2DRef
    g9 = np.load(G9)
    attach(OME)
    OME.set_mode("exact")
    model = make_models(OME, Encoder2DRef, None).MinkUNet34IBN(1, 7, 3)
    assert list(model.state_dict().keys()) == list(g9["keys"])
    model.load_state_dict(seeded_state_dict(model, seed=7))
    model.train()
    coords = torch.from_numpy(g9["coords"])
    threads = torch.get_num_threads()
    torch.set_num_threads(1)   # the fixture was recorded on one thread (BatchNorm sums follow the thread split)
    try:
        with torch.no_grad():
            sem = model(OME.SparseTensor(coordinates=coords, features=torch.ones((coords.shape[0], 1))), is_seg=True)
    finally:
        torch.set_num_threads(threads)
    d = (sem.F - torch.from_numpy(g9["logits"])).abs().max().item()
    assert d <= 5e-5, d


def test_product_model_has_the_reference_keys_shapes_and_size():
    import lidog_amd
    g9 = np.load(G9)
    m = lidog_amd.MinkUNet34IBN(1, 7, 3)
    sd = m.state_dict()
    assert list(sd) == list(g9["keys"])
    for t, s in zip(sd.values(), g9["shapes"]):
        assert list(t.shape) == [int(v) for v in s[:t.dim()]] and not any(s[t.dim():])
    assert sum(p.numel() for p in m.parameters()) == 40004871 == int(g9["n_params"])
    assert len(sd) == 392 and sd["block1.0.in_norm1.weight"].shape == (1, 32)
    assert m.conv0p1s1.kernel.shape[0] == 125     # initial_kernel_size is dropped (ResNetBase): always 5^3


def test_alias_exposes_minkowski_instance_norm():
    code = ("import sys; sys.dont_write_bytecode = True; sys.path.insert(0, %r);"
            "import lidog_amd.me as ME; ME.install_as_minkowski_engine(); import MinkowskiEngine as M;"
            "m = M.MinkowskiInstanceNorm(16);"
            "assert tuple(m.weight.shape) == (1, 16) and float(m.weight.sum()) == 16 and float(m.bias.abs().sum()) == 0;"
            "assert callable(M.ibn_relu); print('ok')" % REPO)
    out = subprocess.run([sys.executable, "-B", "-c", code], capture_output=True, text=True,
                         env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr[-2000:]


def test_convert_sync_batchnorm_leaves_instance_norms_alone():
    import lidog_amd
    import lidog_amd.me as ME
    m = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(lidog_amd.MinkUNet34IBN(1, 7, 3))
    mods = list(m.modules())
    assert sum(isinstance(x, ME.MinkowskiSyncBatchNorm) for x in mods) == 62
    ins = [x for x in mods if isinstance(x, ME.MinkowskiInstanceNorm)]
    assert len(ins) == 9 and not any(isinstance(x, ME.MinkowskiBatchNorm) for x in ins)


def test_train_help_lists_the_ibn_model():
    out = subprocess.run([sys.executable, "-B", "-m", "lidog_amd.train", "--help"], capture_output=True, text=True,
                         cwd=REPO, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert out.returncode == 0 and "MinkUNet34IBN" in out.stdout, out.stderr[-2000:]


def test_instance_norm_entries_in_header_binding_and_exports():
    from lidog_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    header = open(os.path.join(REPO, "include", "lidog_amd.h")).read()
    mine = {n for n in re.findall(r"\b(lidog_i[bn]n?_[a-z0-9_]+)\s*\(", header)}
    assert {"lidog_in_segments", "lidog_in_stats", "lidog_in_apply", "lidog_in_bwd_reduce", "lidog_in_bwd_apply",
            "lidog_ibn_apply", "lidog_ibn_bwd_reduce", "lidog_ibn_bwd_apply", "lidog_in_segments_ws",
            "lidog_in_reduce_ws"} <= mine
    for name in mine:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.lidog_abi_version() == _lib.ABI_VERSION == 9
