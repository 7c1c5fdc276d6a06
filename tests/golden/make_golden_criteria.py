"""Writes tests/golden/g18_criteria.npz: the reference's own criteria (utils/losses/losses.py) on the cases of
tests/ce_ref.py:golden_case, C = 7 and C = 19, 128 rows each with labels 1, 6, every other class and -1 present.

    python tests/golden/make_golden_criteria.py

Per case it records the inputs (logits, labels, weights) and, each with the loss and its gradient w.r.t. the logits,
  ce          CELoss(ignore_label=-1)
  wce         CELoss(ignore_label=-1, weight=weights)
  focal       FocalLoss(alpha=0.25, gamma=2)            (init_losses' arguments; ignore_index stays -1)
  kitti       SoftDICELoss(ignore_label=-1, is_kitti=True)
all run in float32 on the CPU, as the reference runs them.  Needs the reference checkout next to the build."""
import contextlib
import io
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(1, "/root/reference")
import ce_ref as R  # noqa: E402
from utils.losses.losses import CELoss, FocalLoss, SoftDICELoss  # noqa: E402  (reference code)

torch.set_num_threads(1)


def run(crit, x, y):
    x = x.clone().requires_grad_(True)
    loss = crit(x, y)
    loss.backward()
    return loss.detach().numpy(), x.grad.numpy()


def main():
    out = {}
    for C in R.GOLDEN_CLASSES:
        x, y, w = R.golden_case(C)
        assert {1, 6, -1} <= set(y.tolist()) and set(range(C)) <= set(y.tolist())
        with contextlib.redirect_stdout(io.StringIO()):      # CELoss prints its weights
            crits = {"ce": CELoss(ignore_label=-1), "wce": CELoss(ignore_label=-1, weight=w.numpy()),
                     "focal": FocalLoss(alpha=0.25, gamma=2), "kitti": SoftDICELoss(ignore_label=-1, is_kitti=True)}
        out[f"c{C}/logits"], out[f"c{C}/labels"], out[f"c{C}/weights"] = x.numpy(), y.numpy(), w.numpy()
        for name, crit in crits.items():
            loss, grad = run(crit, x, y)
            out[f"c{C}/{name}/loss"], out[f"c{C}/{name}/grad"] = loss, grad
            print(C, name, float(loss), float(np.abs(grad).max()))
    np.savez_compressed(R.G18, **out)
    print(R.G18, os.path.getsize(R.G18), "bytes")


if __name__ == "__main__":
    main()
