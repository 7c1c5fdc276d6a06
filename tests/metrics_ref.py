"""Fixture G17 and the numpy restatement of the per-step training metrics of `log_losses`
(utils/pipelines/trainer_lighting_2d.py:203-291, trainer_lighting.py:118-153).

tests/golden/g17_metrics.npz is written by tests/golden/make_golden_metrics.py with the formulas of those lines:
sklearn's jaccard_score over all rows (the source / mix / SN / RobustNet trainers), a literal confusion-matrix Jaccard on
the rows with label != -1 (what torchmetrics' JaccardIndex computes for the LiDOG trainers) and torch.unique for the
occurrences.  Every case holds `logits` (float32, the shape the trainer sees) and `labels` (int64, -1 = ignore)."""
import os
import re

import numpy as np
import torch

from helpers import GOLDEN, REPO, small_batch

G17 = os.path.join(GOLDEN, "g17_metrics.npz")
C = 7
IGNORE = -1

# name -> (rows or NCHW shape, classes that may be labelled, share of rows labelled -1)
CASES = {
    "points": dict(shape=(4096, C), label_classes=range(7), ignored=0.15),
    "bev": dict(shape=(2, C, 16, 16), label_classes=range(7), ignored=0.3),          # read through .view(b, h, w, -1)
    "absent_class": dict(shape=(1024, C), label_classes=(0, 1, 2, 4, 6), ignored=0.1),
    "all_ignored": dict(shape=(512, C), label_classes=(), ignored=1.0),
}


def make_case(name, seed):
    """(logits float32 of the case's shape, labels int64 [rows])"""
    spec = CASES[name]
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(spec["shape"], generator=g)
    n = logits.numel() // C
    classes = torch.tensor(list(spec["label_classes"]) or [0])
    labels = classes[torch.randint(0, len(classes), (n,), generator=g)]
    labels[torch.rand(n, generator=g) < spec["ignored"]] = IGNORE
    return logits, labels.long()


def rows_of(logits, c=C):
    """the rows the trainers take the arg-max of: [N, C] as it is, NCHW through .view(b, h, w, -1)"""
    return logits.reshape(-1, c)      # of a contiguous tensor: the flat buffer in rows of c


def host_counts(logits, labels, c=C, ignore=IGNORE):
    """[c + 1, c] int64 confusion counts on the host: row 0 = ignored or outside 0..c-1, row l + 1 = label l, column =
    np.argmax of the row (the first maximal index; the first NaN in a row holding one)"""
    x = rows_of(torch.as_tensor(logits), c).numpy()
    lab = np.asarray(labels).reshape(-1)
    out = np.zeros((c + 1, c), np.int64)
    if x.shape[0]:
        pred = np.argmax(x, axis=1)
        row = np.where((lab >= 0) & (lab < c) & (lab != ignore), lab + 1, 0)
        np.add.at(out, (row, pred), 1)
    return out


def kernel_rows_per_block():
    """TS_ROWS of csrc/trainstats.hip"""
    src = open(os.path.join(REPO, "lidog_amd", "csrc", "trainstats.hip")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (TS_THREADS|TS_CHUNKS) (\d+)", src)}
    return d["TS_THREADS"] * d["TS_CHUNKS"]


def scene_batch(seeds, device, n_points=1200, bev=17, seed0=0):
    """a small collated batch with random labels, as tests/test_gpu_train.py's scenes (mapping_bound_2d = 5.0)"""
    coords = small_batch(tuple(seeds), n_points=n_points)
    g = torch.Generator().manual_seed(1000 + seed0 + seeds[0])
    labels = torch.randint(-1, 7, (coords.shape[0],), generator=g)
    bev_labels = torch.randint(-1, 7, (len(seeds), bev, bev), generator=g)
    return {"coords_int": coords.to(device), "source_coordinates0": coords.float().to(device),
            "source_features0": torch.ones((coords.shape[0], 1), device=device),
            "source_sem_labels0": labels.to(device), "source_bev_labels0": {"block8": bev_labels.to(device)}}


class Scenes:
    """scene_batch as a dataset of lidog_amd.train.Fit"""
    config = "scenes"

    def __init__(self, n, seed0=40):
        self.n, self.seed0 = n, seed0

    def __len__(self):
        return self.n

    def batch(self, indices, device):
        return scene_batch([self.seed0 + i for i in indices], device, seed0=self.seed0)
