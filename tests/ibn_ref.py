"""CPU restatement of MinkowskiInstanceNorm (ME 0.5.4, [ME-mem]: from memory, unpinned) and the G9 fixture of the
reference's MinkUNet34IBN (utils/models/minkunet_ibn.py).

The CPU oracle (oracle/me_cpu) has no instance norm, and it is not edited: `attach(OME)` hangs the restatement below on
the oracle module object at run time, so that the reference class -- and lidog_amd.minkunet's wiring bound to the
oracle -- find `ME.MinkowskiInstanceNorm`.  The restatement works in float32 and float64 (model.double()).

G9 (`make_g9`, build container only: it imports the reference) therefore pins the IBN WIRING to the reference class:
module names, call order, shapes, the BN | IN concatenation, the decoder.  It does not pin ME's instance norm itself;
the per-(scan, channel) formulas are the [ME-mem] statement of lidog_amd/me.py (IN_EPS), restated once more, on the
device, by `instance_norm64` for the GPU tests."""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G9 = os.path.join(HERE, "golden", "g9_minkunet34ibn.npz")
EPS = 1e-8          # the [ME-mem] epsilon (lidog_amd.me.IN_EPS)
ADAM_LR, ADAM_WD, ADAM_STEPS = 1e-2, 1e-4, 3     # configs/ibn/*: Adam, lr 0.01; weight decay of the driver


def instance_norm64(x, batch, weight, bias, eps=EPS):
    """y = (x - mean[b]) / sqrt(var[b] + eps) * weight + bias per scan b (biased variance), in the dtype of x (float64
    for the yardstick); autograd-differentiable; x [n, C], batch [n] int, weight / bias [1, C] or [C]."""
    b = batch.long()
    B = int(b.max()) + 1 if b.numel() else 0
    C = x.shape[1]
    cnt = torch.bincount(b, minlength=B).to(x.dtype).clamp_min(1)[:, None]
    mean = torch.zeros((B, C), dtype=x.dtype, device=x.device).index_add(0, b, x) / cnt
    xc = x - mean[b]
    var = torch.zeros((B, C), dtype=x.dtype, device=x.device).index_add(0, b, xc * xc) / cnt
    return xc * torch.rsqrt(var[b] + eps) * weight.reshape(1, C) + bias.reshape(1, C)


def attach(OME):
    """MinkowskiInstanceNorm on the oracle module (CPU): parameters [1, C] ones / zeros, no running statistics"""

    class MinkowskiInstanceNorm(nn.Module):
        def __init__(self, num_features):
            super().__init__()
            self.weight = nn.Parameter(torch.ones(1, num_features))
            self.bias = nn.Parameter(torch.zeros(1, num_features))

        def forward(self, x):
            y = instance_norm64(x.F, x.C[:, 0], self.weight, self.bias)
            return OME.SparseTensor(y, coordinate_manager=x.coordinate_manager, coordinate_map_key=x.coordinate_map_key)

    if not hasattr(OME, "MinkowskiInstanceNorm"):
        OME.MinkowskiInstanceNorm = MinkowskiInstanceNorm
    return OME


def g9_batch():
    """two scans (the G5 / G8 batch of tests/helpers.small_batch) with seeded labels"""
    sys.path.insert(0, HERE)
    from helpers import small_batch
    C = small_batch((0, 1))
    g = torch.Generator().manual_seed(31)
    labels = torch.randint(-1, 7, (C.shape[0],), generator=g)
    return C, labels


def run_model(model_cls, SparseTensor, C, labels, sd, dtype=torch.float32, adam_steps=0, device="cpu"):
    """(model, logits tensor, loss, [losses of adam_steps Adam steps]) of a training-mode forward + backward"""
    from oracle.ref_torch import soft_dice_loss_ref
    model = model_cls(1, 7, 3)
    model.load_state_dict(sd)
    if dtype == torch.float64:
        model.double()
    model.to(device).train()
    feats = torch.ones((C.shape[0], 1), dtype=dtype, device=device)
    sem = model(SparseTensor(coordinates=C.to(device), features=feats), is_seg=True)
    loss = soft_dice_loss_ref(sem.F, labels.to(device))
    loss.backward()
    traj = []
    if adam_steps:
        opt = torch.optim.Adam(model.parameters(), lr=ADAM_LR, weight_decay=ADAM_WD)
        for _ in range(adam_steps):
            opt.step()
            opt.zero_grad()
            s = model(SparseTensor(coordinates=C.to(device), features=feats), is_seg=True)
            lo = soft_dice_loss_ref(s.F, labels.to(device))
            lo.backward()
            traj.append(float(lo.detach()))
    return model, sem, loss, traj


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def make_g9(reference="/root/reference"):
    sys.path.insert(0, REPO)
    sys.path.insert(1, reference)
    import oracle.me_cpu as OME
    from helpers import seeded_state_dict
    OME.install_as_minkowski_engine()
    attach(OME)
    from utils.models.minkunet_ibn import MinkUNet34IBN as RefIBN   # reference code
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    OME.set_mode("exact")
    C, labels = g9_batch()
    sd = seeded_state_dict(RefIBN(1, 7, 3), seed=7)
    m32, sem32, loss32, traj = run_model(RefIBN, OME.SparseTensor, C, labels, sd, adam_steps=ADAM_STEPS)
    m64, sem64, loss64, _ = run_model(RefIBN, OME.SparseTensor, C, labels, sd, dtype=torch.float64)
    p32, p64 = dict(m32.named_parameters()), dict(m64.named_parameters())
    ref_sd = RefIBN(1, 7, 3).state_dict()
    names = list(p64)
    out = dict(coords=C.numpy(), labels=labels.numpy(), keys=np.array(list(ref_sd)),
               shapes=np.array([list(t.shape) + [0] * (4 - t.dim()) for t in ref_sd.values()]),
               n_params=np.int64(sum(p.numel() for p in m32.parameters())),
               logits=sem32.F.detach().numpy(), loss=np.float64(loss32.detach()), adam_losses=np.array(traj),
               logits64=sem64.F.detach().numpy().astype(np.float32),
               logits_err32=np.float64((sem64.F.detach() - sem32.F.detach().double()).abs().max()),
               loss64=np.float64(loss64.detach()), names=np.array(names),
               gnorm=np.array([float(p32[n].grad.norm()) for n in names]) if traj == [] else None,
               gnorm64=np.array([float(p64[n].grad.norm()) for n in names]),
               err32=np.array([_rel(p32[n].grad.numpy(), p64[n].grad.numpy()) for n in names]))
    # gradient norms of the float32 run were taken before the Adam steps changed them: recompute on a fresh model
    m32b, _, _, _ = run_model(RefIBN, OME.SparseTensor, C, labels, sd)
    p32b = dict(m32b.named_parameters())
    out["gnorm"] = np.array([float(p32b[n].grad.norm()) for n in names])
    out["err32"] = np.array([_rel(p32b[n].grad.numpy(), p64[n].grad.numpy()) for n in names])
    np.savez_compressed(G9, **out)
    print("G9", C.shape[0], "loss", float(loss32), "adam", traj, "logits err32", float(out["logits_err32"]),
          "grad err32 max", float(out["err32"].max()))
