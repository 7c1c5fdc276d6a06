"""The G10 fixture of the reference's MinkUNet34Robust (utils/models/minkunet_robustnet.py) and RobustNet's
instance-whitening loss (IWLoss, utils/losses/losses.py:464-485), plus the float64 restatements the tests use.

The CPU oracle (oracle/me_cpu) is not edited.  Two things are hung on the oracle module object at run time:
  - MinkowskiInstanceNorm, by tests/ibn_ref.attach;
  - an in-place MinkowskiReLU (`inplace_relu`, a context manager that restores the oracle's own classes afterwards).
    ME 0.5.4 applies torch.nn.ReLU(inplace=True) to input.F ([ME-mem], lidog_amd.me next to IN_EPS), and the oracle's
    ReLU never works in place.  The reference computes the whitening loss on tensors that its later ReLUs modify, so
    without the substitution the recorded aux values would be those of un-ReLU'd maps.

G10 (`make_g10`, build container only: it imports the reference) records the reference class's logits, SoftDICE, the
five per-map IWLoss values from the reference's own IWLoss (eye and mask built on the CPU the way CovMatrix_IRW builds
them), the epoch-5 total of PLTRobustNet.training_step for one source, a float64 run, gradient norms of the total and a
3-step Adam trajectory."""
import contextlib
import os
import sys

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
G10 = os.path.join(HERE, "golden", "g10_minkunet34robust.npz")
ADAM_LR, ADAM_WD, ADAM_STEPS = 1e-2, 1e-4, 3     # configs/robustnet/*: Adam, lr 0.01; weight decay of the driver
SOURCE_WEIGHTS = (0.5, 0.5)                      # PLTRobustNet's default


def iw_literal(f_map):
    """IWLoss restated literally (utils/losses/losses.py:464-485, eye / mask as CovMatrix_IRW builds them), in the dtype
    and on the device of f_map: [n, C] -> [n, C, 1], per-row outer product / (n - 1) + eps I, * triu(1), |.|, sum / n"""
    n, C = f_map.shape
    eye = torch.eye(C, dtype=f_map.dtype, device=f_map.device)
    mask = torch.ones((C, C), dtype=f_map.dtype, device=f_map.device).triu(1)
    x = f_map.reshape(n, C, 1)
    f_cor = torch.bmm(x, x.transpose(1, 2)).div(n - 1) + 1e-5 * eye
    return torch.sum(torch.sum(torch.abs(f_cor * mask), dim=(1, 2), keepdim=True)) / n


@contextlib.contextmanager
def inplace_relu(OME):
    """MinkowskiReLU(inplace=True) working in place on the oracle (ME 0.5.4's behaviour) while the block runs.

    The reference ReLUs conv1p1s2's output in place after in1 has read it (minkunet_robustnet.py:147-149).  ME's
    instance norm does not keep its input for the backward pass ([ME-mem]); the restatement of tests/ibn_ref.py does
    (index_add), so inside this block the attached MinkowskiInstanceNorm normalises a copy of its input: the same values
    and gradients, and the later in-place ReLU is legal, as in ME."""
    own = OME.MinkowskiReLU
    own_in = OME.MinkowskiInstanceNorm

    class MinkowskiInstanceNorm(own_in):
        def forward(self, x):
            return super().forward(OME.SparseTensor(x.F.clone(), coordinate_manager=x.coordinate_manager,
                                                    coordinate_map_key=x.coordinate_map_key))

    class MinkowskiReLU(nn.Module):
        ACTS_IN_PLACE = True

        def __init__(self, inplace=False):
            super().__init__()
            self.inplace = inplace

        def forward(self, x):
            f = torch.relu_(x.F) if self.inplace else torch.relu(x.F)
            return OME.SparseTensor(f, coordinate_manager=x.coordinate_manager, coordinate_map_key=x.coordinate_map_key)

    OME.MinkowskiReLU, OME.MinkowskiInstanceNorm = MinkowskiReLU, MinkowskiInstanceNorm
    try:
        yield MinkowskiReLU
    finally:
        OME.MinkowskiReLU, OME.MinkowskiInstanceNorm = own, own_in


def step_losses(out, aux_maps, labels, epoch=5):
    """PLTRobustNet.training_step's losses for one source: (sem, [IWLoss per map], aux, total)"""
    from oracle.ref_torch import soft_dice_loss_ref
    sem = soft_dice_loss_ref(out.F, labels)
    per = [iw_literal(m.F) for m in aux_maps]
    aux = sum(p / len(per) for p in per) if epoch >= 5 else torch.zeros((), dtype=sem.dtype)
    total = SOURCE_WEIGHTS[0] * sem + 0.5 * aux
    return sem, per, aux, total


def run_model(model_cls, SparseTensor, C, labels, sd, dtype=torch.float32, adam_steps=0, epoch=5):
    """(model, logits, sem, per-map IW, aux, total, [totals of adam_steps Adam steps]) of a training-mode forward +
    backward of the epoch-`epoch` total"""
    model = model_cls(1, 7, 3)
    model.load_state_dict(sd)
    if dtype == torch.float64:
        model.double()
    model.train()
    feats = torch.ones((C.shape[0], 1), dtype=dtype)
    out, maps = model(SparseTensor(coordinates=C, features=feats), is_seg=False)
    sem, per, aux, total = step_losses(out, maps, labels, epoch)
    total.backward()
    traj = []
    if adam_steps:
        opt = torch.optim.Adam(model.parameters(), lr=ADAM_LR, weight_decay=ADAM_WD)
        for _ in range(adam_steps):
            opt.step()
            opt.zero_grad()
            o, m = model(SparseTensor(coordinates=C, features=feats), is_seg=False)
            t = step_losses(o, m, labels, epoch)[3]
            t.backward()
            traj.append(float(t.detach()))
    return model, out, sem, per, aux, total, traj


def make_g10(reference):
    sys.path.insert(0, REPO)
    sys.path.insert(1, reference)
    import oracle.me_cpu as OME
    from helpers import seeded_state_dict
    from ibn_ref import _rel, attach, g9_batch
    OME.install_as_minkowski_engine()
    attach(OME)
    from utils.models.minkunet_robustnet import MinkUNet34Robust as RefRobust   # reference code
    from utils.losses.losses import IWLoss as RefIWLoss                          # reference code
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    OME.set_mode("exact")
    C, labels = g9_batch()
    with inplace_relu(OME) as relu_cls:
        sd = seeded_state_dict(RefRobust(1, 7, 3), seed=7)
        probe = RefRobust(1, 7, 3)
        active = isinstance(probe.relu, relu_cls) and probe.relu.inplace
        m32, out32, sem32, per32, aux32, tot32, traj = run_model(RefRobust, OME.SparseTensor, C, labels, sd,
                                                                 adam_steps=ADAM_STEPS)
        m64, out64, sem64, per64, aux64, tot64, _ = run_model(RefRobust, OME.SparseTensor, C, labels, sd,
                                                              dtype=torch.float64)
        m32b, _, _, _, _, _, _ = run_model(RefRobust, OME.SparseTensor, C, labels, sd)
        # the per-map values again, from the reference's own IWLoss on the reference model's aux maps
        m = RefRobust(1, 7, 3)
        m.load_state_dict(sd)
        m.train()
        with torch.no_grad():
            _, maps = m(OME.SparseTensor(coordinates=C, features=torch.ones((C.shape[0], 1))), is_seg=False)
        ref_iw = RefIWLoss()
        per_ref = []
        for t in maps:
            dim = t.F.shape[1]
            eye, mask = torch.eye(dim, dim), torch.ones(dim, dim).triu(diagonal=1)    # CovMatrix_IRW, on the CPU
            margin = torch.sum(mask) // 2.0
            per_ref.append(float(ref_iw(t.F, eye, mask, margin, torch.sum(mask))))
        aux_min = [float(t.F.min()) for t in maps]
    assert active, "the in-place ReLU substitution was not active"
    p64, p32b = dict(m64.named_parameters()), dict(m32b.named_parameters())
    ref_sd = RefRobust(1, 7, 3).state_dict()
    names = list(p64)
    out = dict(coords=C.numpy(), labels=labels.numpy(), keys=np.array(list(ref_sd)),
               shapes=np.array([list(t.shape) + [0] * (4 - t.dim()) for t in ref_sd.values()]),
               n_params=np.int64(sum(p.numel() for p in m32.parameters())),
               inplace_relu=np.bool_(active), aux_min=np.array(aux_min),
               logits=out32.F.detach().numpy(), sem=np.float64(sem32.detach()),
               iw=np.array([float(p.detach()) for p in per32]), iw_ref=np.array(per_ref),
               aux=np.float64(aux32.detach()), total=np.float64(tot32.detach()), adam_losses=np.array(traj),
               logits64=out64.F.detach().numpy().astype(np.float32),
               logits_err32=np.float64((out64.F.detach() - out32.F.detach().double()).abs().max()),
               sem64=np.float64(sem64.detach()), iw64=np.array([float(p.detach()) for p in per64]),
               total64=np.float64(tot64.detach()), names=np.array(names),
               gnorm=np.array([float(p32b[n].grad.norm()) for n in names]),
               gnorm64=np.array([float(p64[n].grad.norm()) for n in names]),
               err32=np.array([_rel(p32b[n].grad.numpy(), p64[n].grad.numpy()) for n in names]))
    np.savez_compressed(G10, **out)
    print("G10", C.shape[0], "sem", float(sem32.detach()), "iw", out["iw"].tolist(), "iw_ref", per_ref, "total",
          float(tot32.detach()), "adam", traj, "aux min", aux_min, "grad err32 max", float(out["err32"].max()))
