"""The owning training driver: model -> data-parallel wiring -> epochs of steps -> validation -> checkpoints.

What the reference's entry scripts do through pytorch-lightning, as plain arguments (no YAML engine):
  get_model / SyncBN + DDP / Trainer args   train_lidog.py:42-75,227-231,286-296 (train_source.py:43-58,196-234,
                                            train_aug_based.py:44-53,189-230)
  ModelCheckpoint(every_n_epochs=1, save_on_train_epoch_end, save_top_k=-1)          train_lidog.py:222-225
  Trainer(max_epochs, check_val_every_n_epoch, num_sanity_val_steps=2), fit(ckpt_path=resume)   :286-301
  DistributedSampler sharding + per-epoch reshuffle (what Lightning injects under strategy='ddp', shuffle=True :186)
  epoch-interval scheduler stepping (configure_optimizers returns ([optimizer], [scheduler]))

    python -m lidog_amd.train --model MinkUNet34BEV --epochs 2 --scans 16 --batch 4 --save-dir /tmp/run
    python -m torch.distributed.run --nproc-per-node N -m lidog_amd.train ...        (one process per GPU, RCCL)
    python -m lidog_amd.train --sources kitti120k nusc35k --source-weights 0.5 0.5 ...   (two sources, */multi/*.yaml)
    python -m lidog_amd.train --model MinkUNet34 --mix cosmix ...    (PointCutMix / CoSMix, configs/{pointcutmix,cosmix})
    python -m lidog_amd.train --model MinkUNet34 --mix polarmix --mix-instance-classes 0 1 ...   (PolarMix)
    python -m lidog_amd.train --model MinkUNet34 --mix lasermix --mix-pitch -25 3 ...   (LaserMix; neither is in the reference)
    python -m lidog_amd.train --model MinkUNet34 --mix cosmix --source-augment RandomRotation RandomScale ...
                                              (the source datasets' augmentation_list under --mix / --mix3d / --sn-targets)
    python -m lidog_amd.train --model MinkUNet34 --config kitti120k_cars --sn-targets nusc35k_cars ...   (SN, configs/SN)
    python -m lidog_amd.train --augment RandomRotation RandomScale --sub-p 0.8 ...   (sub_p / augmentation_list of the configs)
    python -m lidog_amd.train --log-every-n-steps 50 --save-dir /tmp/run ...   (per-step IoU, class counts, losses, lr ->
                                                                       /tmp/run/metrics.jsonl: lidog_amd.metrics)
    python -m lidog_amd.train --files SemanticKITTI=/data/SemanticKITTI --label-maps semantickitti2common.yaml ...
                                                                       (scans from files: lidog_amd.scans)
    python -m lidog_amd.train --model MinkUNet34 --config kitti120k --raycast-to nusc35k --lr 0.01 --scheduler ExponentialLR
                                              (the Raycast baseline, configs/raycast: lidog_amd.raycast)

Scans are synthetic (lidog_amd.synth; there are no datasets on the box) unless --files names a dataset on disk
(lidog_amd.scans: SemanticKITTI, Synth4D, a nuScenes pair list); anything with `__len__` and
`batch(indices, device) -> dict` (keys of CollateFNSingleSourceBEVMultiLevel, collation.py:318-325) can be passed as
`train_data` / `val_data` instead.
"""
import argparse
import functools
import os
import re

import numpy as np
import torch
import torch.distributed as dist

from . import me as ME
from . import scans
from . import synth
from .checkpoint import load_training_checkpoint, save_lightning_checkpoint
from .data import (MIXSTYLE_DEFAULT_STAGES, augment_item, band_bounds, check_augmentations, check_mixstyle_arguments,
                   collate_items, cosmix_merge, draw_augmentation,
                   draw_lasermix, draw_polarmix, draw_scaling, draw_source, instance_mask, lasermix_merge, mix3d_merge,
                   on_merge_stream, pointcutmix_merge, polarmix_merge, scaling_params, sn_scale)
from . import precision as _precision
from .evaluate import CLASS_NAMES, per_class_iou
from .losses import AUX_CRITERIA, BEV_CRITERIA, POINT_CRITERIA
from .metrics import MetricLayout, MetricsWriter, StepMetrics
from . import optim as _optim
from .optim import SAM, WeightAverage, check_sam_arguments, make_optimizer, make_scheduler, shard_indices
from .trainer import LiDOGStep, RobustStep, SourceStep, setup_data_parallel


class SynthScans:
    """`n` synthetic scans of one configuration; scan i = seed `first + i` (SURVEY.md 8(d) generator)"""

    def __init__(self, n, config="kitti120k", first=0, mix3d=False, bev_size=167):
        self.n, self.config, self.first, self.mix3d, self.bev_size = n, config, first, mix3d, bev_size

    def __len__(self):
        return self.n

    def batch(self, indices, device):
        return synth.make_batch([self.first + i for i in indices], self.config, device, bev_size=self.bev_size,
                                mix3d=self.mix3d)


class MultiSynthScans:
    """Two sources paired as MultiBEVSourceDataset (utils/datasets/synth4d_bev.py:682-772): the length is the larger of
    the two; item i takes scan i of source 0 and scan perm[i] of source 1 (perm: a permutation of source 1 shuffled once
    at construction); an index past a source's end takes a random scan of that source.  The permutation and the random
    draws come from `seed` (the run's seed): the same seed gives the same pairs in the same order.  Source 1's scans
    have their own seed range (synth.SOURCE1_SEED), so one configuration on both sources gives two sets of scans."""

    num_sources = 2

    def __init__(self, n0, n1, configs=("kitti120k", "nusc35k"), seed=1234, first=0, mix3d=False, bev_size=167):
        if len(configs) != 2:
            raise NotImplementedError(f"{len(configs)} sources (the reference takes one or two)")
        self.n = (int(n0), int(n1))
        self.configs, self.first, self.mix3d, self.bev_size = tuple(configs), first, mix3d, bev_size
        rng = np.random.default_rng([int(seed), 2])
        self.perm1 = rng.permutation(self.n[1])
        self._draws = np.random.default_rng([int(seed), 3])

    def __len__(self):
        return max(self.n)

    def pair(self, i):
        """(index into source 0, index into source 1) of item i"""
        j0 = i if i < self.n[0] else int(self._draws.integers(0, self.n[0]))
        j1 = int(self.perm1[i]) if i < self.n[1] else int(self._draws.integers(0, self.n[1]))
        return j0, j1

    def batch(self, indices, device):
        pairs = [self.pair(i) for i in indices]
        return synth.make_batch([self.first + a for a, _ in pairs], self.configs[0], device, bev_size=self.bev_size,
                                mix3d=self.mix3d, seeds1=[self.first + b for _, b in pairs], config1=self.configs[1])


class PlainSynthItems:
    """The item provider of MixedSynthScans / ScaledSynthScans over plain synthetic voxel scans (the default): an item is
    the scan as it is and draws nothing, the reference's `if self.phase == 'train' and self.augmentations is not None`
    with a null augmentation_list.  A provider has `augmentations` (the source datasets' list or None), `sub_p`,
    `voxel`, `draw_item(s, j, rng, device)` (host draws of scan j of source s, in the reference's __getitem__ sequence),
    `make_item(s, j, draws, device)` (the item as the merges read it, on the device), `class_weights(n, num_classes)` and
    `face_name(s)`.  AugmentedSynthScans and scans.FileScans are the other two."""

    augmentations = None
    sub_p = None

    def __init__(self, configs, first=0):
        self.configs, self.first = tuple(configs), int(first)
        self.voxel = synth.CONFIGS[self.configs[0]]["voxel"]

    def draw_item(self, s, j, rng, device=None):
        return None

    def make_item(self, s, j, draws, device):
        vox, labels = synth.scan_voxels(self.first + j + s * synth.SOURCE1_SEED, self.configs[s])
        return {"coordinates": torch.from_numpy(vox).to(device),
                "features": torch.ones((vox.shape[0], 1), dtype=torch.float32, device=device),
                "sem_labels": torch.from_numpy(labels).to(device)}

    def class_weights(self, n, num_classes=7):
        return tuple(source_class_counts(c, [self.first + j + s * synth.SOURCE1_SEED for j in range(k)], num_classes)
                     for s, (c, k) in enumerate(zip(self.configs, n)))

    def face_name(self, s):
        return synth.CONFIGS[self.configs[s]].get("dataset", self.configs[s])


def merge_scan(item, j):
    """an item of augment_item as the merges and sn_scale read it: the reference's keys, `idx` the scan's index"""
    scan = {k: item[k] for k in ("coordinates", "features", "sem_labels", "xyz", "sampled_idx")}
    scan["idx"] = torch.tensor(int(j))
    return scan


class MixedSynthScans:
    """Mix3DSourceDataset / PointCutMixSourceDataset / CoSMixSourceDataset (utils/datasets/mix3D.py, pointcutmix.py,
    cosmix.py; train_aug_based.py:86-102): two sources paired as MultiSynthScans.pair, each item ONE scan merged from its
    pair on the GPU (lidog_amd.data.mix3d_merge / pointcutmix_merge / cosmix_merge), so a batch is a one-source batch
    (num_sources = 1) with the keys SourceStep reads.  The two scans come from an item provider (`items`): plain synthetic
    voxel scans (PlainSynthItems, the default), the augmented items of an AugmentedSynthScans, or the items of a
    scans.FileScans.  Item i of epoch e draws from ONE np.random.RandomState([seed, e, i]) in the order of the
    reference's __getitem__: source 0's item, source 1's item, then the merge's own draws, CoSMix applying the
    provider's augmentation list once more to every pasted class: a mix does not depend on the world size, the batch
    split or a resume (Fit calls set_epoch).  `plan(i)` gives the host side of that.  The scans are uploaded and merged
    on data.merge_stream, and the batch is handed to the caller's stream with an event: the merges' read-backs do not
    wait for a training step queued earlier.  CoSMix's class weights are the per-class label counts over each source's
    training scans (get_dataset_stats, synth4d.py:203-220; FileScans.class_counts over files); the voxel size is source
    0's, as the reference's.  SENSOR_METHODS (polarmix, lasermix) are the two sensor-aware mixes, which the reference
    does not have: `instance_classes` are the classes PolarMix pastes, `pitch` (degrees) and `areas` the vertical field
    of view and the band counts LaserMix draws from."""

    num_sources = 1
    METHODS = ("pointcutmix", "cosmix")
    ALL_METHODS = ("mix3d",) + METHODS
    # PolarMix / LaserMix (lidog_amd.data.polarmix_merge / lasermix_merge): not in the reference.  Their draws need no
    # device counts, so plan(i)["merge"] holds all of them.
    SENSOR_METHODS = ("polarmix", "lasermix")

    def __init__(self, n0, n1, configs=("kitti120k", "kitti120k"), method="cosmix", sub_p=0.8, seed=1234, first=0,
                 num_classes=7, items=None, pitch=(-25.0, 3.0), instance_classes=(0, 1), areas=(3, 4, 5, 6)):
        if method not in self.ALL_METHODS + self.SENSOR_METHODS:
            raise NotImplementedError(f"mixing method {method!r} (one of {self.ALL_METHODS + self.SENSOR_METHODS})")
        self.pitch, self.instance_classes, self.areas = tuple(pitch), tuple(instance_classes), tuple(areas)
        self.items = PlainSynthItems(configs, first) if items is None else items
        self.pairs = MultiSynthScans(n0, n1, configs, seed=seed, first=first)
        self.configs, self.method, self.seed, self.first = tuple(configs), method, int(seed), first
        # the reference's self.sub_p / self.augmentations = source_dataset0's; plain scans keep the constructor's sub_p
        self.sub_p = sub_p if items is None else self.items.sub_p
        self.augmentations = self.items.augmentations
        self.voxel = self.items.voxel
        self.epoch = 0
        if method == "mix3d":
            self.merge = lambda s0, s1, rng: mix3d_merge(s0, s1, voxel_size=self.voxel)
        elif method == "pointcutmix":
            self.merge = functools.partial(pointcutmix_merge, voxel_size=self.voxel)
        elif method == "polarmix":
            instance_mask(self.instance_classes)      # ValueError for a class outside 0 .. 31
            self.merge = functools.partial(polarmix_merge, instance_classes=self.instance_classes)
        elif method == "lasermix":
            for n_areas in self.areas:
                band_bounds(self.pitch, n_areas)      # ValueError for a bad pitch range or band count
            self.merge = functools.partial(lasermix_merge, pitch=self.pitch, areas=self.areas)
        else:
            self.class_weights = tuple(self.items.class_weights((int(n0), int(n1)), num_classes))
            self.merge = functools.partial(cosmix_merge, voxel_size=self.voxel, class_weights=self.class_weights,
                                           sub_p=self.sub_p, augmentations=self.augmentations)

    def __len__(self):
        return len(self.pairs)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def item_rng(self, i):
        return np.random.RandomState([self.seed, self.epoch, int(i)])

    def _draws(self, i, device=None):
        """(scan indices, the two items' draws, the generator standing at the merge's first draw)"""
        rng = self.item_rng(i)
        js = self.pairs.pair(i)
        return js, [self.items.draw_item(s, j, rng, device) for s, j in enumerate(js)], rng

    def plan(self, i, device=None):
        """the host side of item i in the current epoch: {'scans': (j0, j1), 'items': [draws of source 0's item, of
        source 1's] (None: an item that draws nothing), 'merge': {'source': the merge's first draw} (mix3d: {})}.  The
        merge's later draws (cells, classes, sub-samples, per-class transforms) follow from the same generator but
        depend on counts the device makes from the two items; polarmix / lasermix need no counts, and 'merge' is the
        whole dict of draw_polarmix / draw_lasermix.  Synthetic providers need no device; a FileScans
        provider reads the scan's point count from the loaded file."""
        js, draws, rng = self._draws(i, device)
        if self.method == "polarmix":
            merge = draw_polarmix(rng)
        elif self.method == "lasermix":
            merge = draw_lasermix(rng, self.areas)
        else:
            merge = {} if self.method == "mix3d" else {"source": draw_source(rng)}
        return {"scans": tuple(js), "items": draws, "merge": merge}

    def _scan(self, s, j, device):
        return self.items.make_item(s, j, None, device)

    def _item(self, i, device):
        js, draws, rng = self._draws(i, device)
        scans_ = [self.items.make_item(s, j, d, device) for s, (j, d) in enumerate(zip(js, draws))]
        return self.merge(scans_[0], scans_[1], rng=rng)

    def item(self, i, device="cuda"):
        """the merged dict of item i in the current epoch (the merge's keys)"""
        device = torch.device(device)
        return on_merge_stream(lambda: self._item(i, device), device, wait=False)

    def _batch(self, indices, device):
        coords, feats, labels = [], [], []
        for b, i in enumerate(indices):
            m = self._item(i, device)
            c = m["coordinates"].to(torch.int32)
            coords.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int32, device=c.device), c], dim=1))
            feats.append(m["features"])
            labels.append(m["sem_labels"].long())
        coords = torch.cat(coords)
        return {"coords_int": coords, "source_coordinates0": coords.float(), "source_features0": torch.cat(feats),
                "source_sem_labels0": torch.cat(labels)}

    def batch(self, indices, device):
        device = torch.device(device)
        if device.type != "cuda":
            return self._batch(indices, device)
        # the scans are made on the merge stream itself: it does not wait for the caller's stream
        return on_merge_stream(lambda: self._batch(indices, device), device, wait=False)


class SynthDataset:
    """the face of a reference dataset that the SN statistics read (train_scaling_based.py:35-87): `name`, `voxel_size`,
    `len` and items with `coordinates` and `sem_labels`, over `n` synthetic scans (scan i = seed `first + i`).  The name
    is the configuration's `dataset` when it has one ('NuScenesDataset' switches get_average_dims' thresholds)."""

    def __init__(self, n, config, first=0):
        self.n, self.config, self.first = int(n), config, int(first)
        self.name = synth.CONFIGS[config].get("dataset", config)
        self.voxel_size = synth.CONFIGS[config]["voxel"]
        self.ignore_label = -1

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        vox, labels = synth.scan_voxels(self.first + int(i), self.config)
        return {"coordinates": torch.from_numpy(vox), "sem_labels": torch.from_numpy(labels)}


class ItemFace:
    """the same face over the items of an item provider (source s): item i is made with draws taken from `rng`, the
    generator average_dims is given, so the sequence is draw_scans first, then every selected item's own draws
    (get_average_dims reads `dataset.__getitem__(i)` of the augmented training dataset, train_scaling_based.py:44-46)"""

    def __init__(self, items, s, n, rng, device="cuda"):
        self.items, self.s, self.n, self.rng, self.device = items, int(s), int(n), rng, torch.device(device)
        self.name, self.voxel_size, self.ignore_label = items.face_name(s), items.voxel, -1

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        draws = self.items.draw_item(self.s, int(i), self.rng, self.device)
        item = on_merge_stream(lambda: self.items.make_item(self.s, int(i), draws, self.device), self.device, wait=False)
        return {"coordinates": item["coordinates"], "sem_labels": item["sem_labels"]}


class ScaledSynthScans:
    """SingleSNSourceDataset / MultiSNSourceDataset (utils/datasets/sn_scaling.py; train_scaling_based.py:253-264) over
    synthetic scans: every item is a source scan whose coordinates are scaled per axis by (target car size / source car
    size) and re-quantised on the GPU (lidog_amd.data.sn_scale).  One source: a one-source batch with the keys
    SourceStep reads; two sources: paired as MultiSynthScans.pair, a two-source batch.
    The car sizes are computed once, here, on the device (lidog_amd.data.average_dims over the `n` training scans of
    every source, then over `n_target` scans of every target, which start at scan 10^6 as the validation scans do: the
    reference takes its targets' validation split), with the draws of np.random.RandomState(seed); `scaling` (the list
    scaling_params returns) skips that.  Quirks kept: with ONE source the first target's row is always applied
    (sn_scaling.py:46-51 tests the number of sources); with two, each item draws one target row per source.  Item i of
    epoch e draws from np.random.RandomState([seed, e, i]), as MixedSynthScans: a batch does not depend on the world
    size, the batch split or a resume.
    `items`: an item provider as MixedSynthScans takes (default: the plain voxel scans).  An item then draws, from that
    one generator, source 0's item, source 1's item, then the scale rows (sn_scaling.py:36-51,107-131), and the source
    statistics are taken on the provider's (augmented) training items, the targets' on their plain validation items
    (`target_faces`: ready-made dataset faces, for targets read from files).  `plan(i)` is the host side of an item."""

    def __init__(self, n, configs, targets, seed=1234, first=0, n_target=None, scaling=None, device="cuda",
                 cache_dir=None, items=None, target_faces=None):
        configs = (configs,) if isinstance(configs, str) else tuple(configs)
        if len(configs) not in (1, 2):
            raise NotImplementedError(f"{len(configs)} sources (the reference takes one or two)")
        if not targets and not target_faces:
            raise ValueError("ScaledSynthScans needs at least one target configuration")
        self.configs, self.targets = configs, tuple(targets)
        self.num_sources = len(configs)
        ns = tuple(int(k) for k in n) if isinstance(n, (tuple, list)) else (int(n),) * self.num_sources
        if len(ns) != self.num_sources:
            raise ValueError("n: one number of scans, or one per source")
        n = max(ns)
        self.n, self.seed, self.first, self.epoch = n, int(seed), int(first), 0
        self.pairs = MultiSynthScans(ns[0], ns[1], configs, seed=seed, first=first) if self.num_sources == 2 else None
        self.items = PlainSynthItems(configs, first) if items is None else items
        self.voxel = self.items.voxel                        # the reference's self.voxel_size = source_dataset0.voxel_size
        if scaling is None:
            rng = np.random.RandomState(self.seed)
            if items is None:
                sources = [SynthDataset(ns[s], c, first + s * synth.SOURCE1_SEED) for s, c in enumerate(configs)]
            else:
                sources = [ItemFace(items, s, ns[s], rng, device) for s in range(self.num_sources)]
            tgts = list(target_faces) if target_faces else [
                SynthDataset(n if n_target is None else n_target, c, 10 ** 6 + t * synth.SOURCE1_SEED)
                for t, c in enumerate(self.targets)]
            scaling = scaling_params(sources, tgts, cache_dir=cache_dir, rng=rng, device=device)
        self.scaling = [np.asarray(a, dtype=np.float32) for a in scaling]
        if len(self.scaling) != self.num_sources or any(a.ndim != 2 or a.shape[1] != 3 for a in self.scaling):
            raise ValueError("scaling: one [n_targets, 3] array per source")

    def __len__(self):
        return self.n

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def item_rng(self, i):
        return np.random.RandomState([self.seed, self.epoch, int(i)])

    def plan(self, i, device=None):
        """the host side of item i in the current epoch: {'scans': scan indices, 'items': [draws of each source's item]
        (None: an item that draws nothing), 'merge': {'rows': the scale row of each source}}, drawn in that order"""
        rng = self.item_rng(i)
        js = (int(i),) if self.pairs is None else self.pairs.pair(i)
        draws = [self.items.draw_item(s, j, rng, device) for s, j in enumerate(js)]
        return {"scans": tuple(js), "items": draws, "merge": {"rows": draw_scaling(rng, self.scaling, self.num_sources)}}

    def item(self, i):
        """[(source, scan index, scale row)] of item i in the current epoch"""
        p = self.plan(i)
        return [(s, j, p["merge"]["rows"][s]) for s, j in enumerate(p["scans"])]

    def scan(self, s, j, device, draws=None):
        return self.items.make_item(s, j, draws, device)

    scale = staticmethod(sn_scale)

    def _batch(self, indices, device):
        cols = [([], [], []) for _ in range(self.num_sources)]
        for b, i in enumerate(indices):
            p = self.plan(i, device)
            for s, (j, draws, row) in enumerate(zip(p["scans"], p["items"], p["merge"]["rows"])):
                m = self.scale(self.scan(s, j, device, draws), row, voxel_size=self.voxel)
                c = m["coordinates"].to(torch.int32)
                cols[s][0].append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int32, device=c.device), c],
                                            dim=1))
                cols[s][1].append(m["features"])
                cols[s][2].append(m["sem_labels"].long())
        batch = {}
        for s, (coords, feats, labels) in enumerate(cols):
            coords = torch.cat(coords)
            batch["coords_int1" if s else "coords_int"] = coords
            batch.update({f"source_coordinates{s}": coords.float(), f"source_features{s}": torch.cat(feats),
                          f"source_sem_labels{s}": torch.cat(labels)})
        return batch

    def batch(self, indices, device):
        device = torch.device(device)
        if device.type != "cuda":
            return self._batch(indices, device)
        # the scans are made on the merge stream itself: it does not wait for the caller's stream
        return on_merge_stream(lambda: self._batch(indices, device), device, wait=False)


class AugmentedSynthScans:
    """A training dataset with `sub_p` and a non-null `augmentation_list` (25 of the reference's 48 configurations:
    semantickitti_bev.py:209-252, synth4d.py:141-162) over synthetic scans: every item is made from the scan's POINTS
    (synth.scan_points_labels) each time it is asked for: a random int(sub_p * n) of them in random order, rotated and
    scaled, voxelised on the GPU (lidog_amd.data.augment_item).  `bev=(bound, image size)` is the BEV datasets' form:
    the bounds filter with the ego box, and BEV label images rasterised from the voted labels; without it neither
    (Synth4DDataset).  One configuration: a one-source batch; two: paired as MultiSynthScans.pair, each source's item
    augmented on its own, source 0 first (MultiBEVSourceDataset.__getitem__).  The draws of item i in epoch e come from
    np.random.RandomState([seed, e, i]) in the reference's sequence: a batch does not depend on the world size, the
    batch split or a resume (Fit calls set_epoch).  Items are made on data.merge_stream.
    `raycast` (a raycast.SensorSpec, a sensor's name or JSON file): the Raycast baseline.  Every scan is resampled to
    that sensor on the GPU (lidog_amd.raycast.raycast_scan) before anything is drawn, as seen from `raycast_origin`
    (default: raycast.origin_between(configuration, sensor) when the sensor is a configuration's, else 0); the draws see
    the resampled point count.  Only then may `augmentations` be None: nothing is drawn, every point in order, as
    scans.FileScans.draws."""

    CACHE_SCANS = 256

    def __init__(self, n, configs, augmentations, sub_p=0.8, seed=1234, first=0, bev=None, ignore_label=-1,
                 raycast=None, raycast_origin=None):
        configs = (configs,) if isinstance(configs, str) else tuple(configs)
        if len(configs) not in (1, 2):
            raise NotImplementedError(f"{len(configs)} sources (the reference takes one or two)")
        self.configs, self.num_sources = configs, len(configs)
        self.raycast, self.raycast_origins = None, None
        if raycast is not None:
            from . import raycast as _raycast
            self.raycast = _raycast.sensor(raycast)
            between = self.raycast.name in synth.CONFIGS
            self.raycast_origins = [raycast_origin if raycast_origin is not None else
                                    (_raycast.origin_between(c, self.raycast.name) if between else None) for c in configs]
        self.augmentations = None if (augmentations is None and raycast is not None) else \
            check_augmentations(augmentations)
        self.sub_p, self.bev, self.ignore_label = sub_p, bev, ignore_label
        self.n, self.seed, self.first, self.epoch = int(n), int(seed), int(first), 0
        self.pairs = MultiSynthScans(n, n, configs, seed=seed, first=first) if self.num_sources == 2 else None
        self._cache = {}

    def __len__(self):
        return self.n

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def item_rng(self, i):
        return np.random.RandomState([self.seed, self.epoch, int(i)])

    def points(self, s, j):
        """(points, labels) of scan j of source s, on the host (kept, as the reference's use_cache)"""
        if (s, j) not in self._cache:
            if len(self._cache) >= self.CACHE_SCANS:
                self._cache.clear()
            self._cache[(s, j)] = synth.scan_points_labels(self.first + j + s * synth.SOURCE1_SEED, self.configs[s])
        return self._cache[(s, j)]

    def scan(self, s, j, device):
        """the scan dict of scan j of source s on `device`, uploaded (and with `raycast` resampled) on the current
        stream"""
        pts, labels = self.points(s, j)
        scan = {"points": torch.from_numpy(pts).to(device), "sem_labels": torch.from_numpy(labels).to(device),
                "features": torch.ones((pts.shape[0], 1), dtype=torch.float32, device=device)}
        if self.raycast is not None:
            from .raycast import raycast_scan
            scan = raycast_scan(scan, self.raycast, self.raycast_origins[s])
        return scan

    def draws(self, rng, m):
        """the draws of one item of m points: the reference's sequence with an augmentation list, nothing otherwise"""
        if self.augmentations is None:
            return {"sampled_idx": np.arange(m), "ops": []}
        return draw_augmentation(rng, m, self.sub_p, self.augmentations)

    def item(self, i):
        """[(source, scan index, draws)] of item i in the current epoch (without `raycast`: with it the number of
        points is known on the device only, see _batch)"""
        if self.raycast is not None:
            raise RuntimeError("item: with raycast the draws follow the resampled scan, ask for batch()")
        rng = self.item_rng(i)
        js = (int(i),) if self.pairs is None else self.pairs.pair(i)
        return [(s, j, draw_augmentation(rng, self.points(s, j)[0].shape[0], self.sub_p, self.augmentations))
                for s, j in enumerate(js)]

    # ---- the item provider of MixedSynthScans / ScaledSynthScans (see PlainSynthItems)
    @property
    def voxel(self):
        return synth.CONFIGS[self.configs[0]]["voxel"]

    def draw_item(self, s, j, rng, device=None):
        if self.raycast is not None:    # the resampled point count is known once the scan is on the device
            device = torch.device("cuda" if device is None else device)
            scan = on_merge_stream(lambda: self.scan(s, j, device), device, wait=False)
            self._last = ((s, int(j), str(device)), scan)
            return self.draws(rng, scan["points"].shape[0])
        return draw_augmentation(rng, self.points(s, j)[0].shape[0], self.sub_p, self.augmentations)

    def make_item(self, s, j, draws, device):
        if self.raycast is not None:
            device = torch.device(device)
            key, scan = getattr(self, "_last", (None, None))
            if key != (s, int(j), str(device)):
                scan = self.scan(s, j, device)
            self._last = (None, None)
            return merge_scan(augment_item(scan, draws, voxel_size=synth.CONFIGS[self.configs[s]]["voxel"],
                                           bounds=self.bev is not None, ignore_label=self.ignore_label), j)
        pts, labels = self.points(s, j)
        scan = {"points": torch.from_numpy(pts).to(device), "sem_labels": torch.from_numpy(labels).to(device),
                "features": torch.ones((pts.shape[0], 1), dtype=torch.float32, device=device)}
        return merge_scan(augment_item(scan, draws, voxel_size=synth.CONFIGS[self.configs[s]]["voxel"],
                                       bounds=self.bev is not None, ignore_label=self.ignore_label), j)

    def class_weights(self, n, num_classes=7):
        """get_dataset_stats: per-class counts of the labels of ALL points of each source's training scans"""
        out = []
        for s, k in enumerate(n):
            w = np.zeros(num_classes)
            for j in range(k):
                lab = self.points(s, j)[1]
                w += np.bincount(lab[(lab >= 0) & (lab < num_classes)], minlength=num_classes)
            out.append(w)
        return tuple(out)

    def face_name(self, s):
        return synth.CONFIGS[self.configs[s]].get("dataset", self.configs[s])

    def _raycast_batch(self, indices, device):
        items = []
        for i in indices:
            rng = self.item_rng(i)
            row = []
            for s, j in enumerate((int(i),) if self.pairs is None else self.pairs.pair(i)):
                scan = self.scan(s, j, device)
                row.append(augment_item(scan, self.draws(rng, scan["points"].shape[0]),
                                        voxel_size=synth.CONFIGS[self.configs[s]]["voxel"], bounds=self.bev is not None,
                                        ignore_label=self.ignore_label, bev=self.bev))
            items.append(row)
        return collate_items(items, self.bev is not None)

    def _batch(self, indices, device):
        if self.raycast is not None:
            return self._raycast_batch(indices, device)
        items = []
        for i in indices:
            row = []
            for s, j, draws in self.item(i):
                pts, labels = self.points(s, j)
                scan = {"points": torch.from_numpy(pts).to(device), "sem_labels": torch.from_numpy(labels).to(device),
                        "features": torch.ones((pts.shape[0], 1), dtype=torch.float32, device=device)}
                row.append(augment_item(scan, draws, voxel_size=synth.CONFIGS[self.configs[s]]["voxel"],
                                        bounds=self.bev is not None, ignore_label=self.ignore_label, bev=self.bev))
            items.append(row)
        return collate_items(items, self.bev is not None)

    def batch(self, indices, device):
        device = torch.device(device)
        # the scans are uploaded on the merge stream itself: it does not wait for the caller's stream
        return on_merge_stream(lambda: self._batch(indices, device), device, wait=False)


def source_class_counts(config, seeds, num_classes=7):
    """Synth4DDataset.get_dataset_stats (synth4d.py:203-220) over synthetic scans: per-class label counts, the ignore
    label (-1) left out"""
    w = np.zeros(num_classes)
    for s in seeds:
        _, labels = synth.scan_voxels(s, config)
        lbl, count = np.unique(labels, return_counts=True)
        keep = (lbl >= 0) & (lbl < num_classes)
        w[lbl[keep]] += count[keep]
    return w


def source_names(configs):
    """keys of the per-source validation results: the configuration names, made unique by their position"""
    return [c if list(configs).count(c) == 1 else f"{c}:{i}" for i, c in enumerate(configs)]


def training_source_names(data, num_sources):
    """the names the training metrics file a dataset's sources under: its configurations (`configs` / `config`) or its
    listings' names, made unique by source_names; `source<s>` for a dataset that has neither"""
    names = getattr(data, "configs", None)
    if names is None and hasattr(data, "config"):
        names = [data.config]
    if names is None and hasattr(data, "listings"):
        names = [l.name for l in data.listings]
    names = list(names or [])[:num_sources]
    names += [f"source{s}" for s in range(len(names), num_sources)]
    return source_names(names)


def bev_image_size(bound_2d, voxel=0.05, pool=(5, 3, 1)):
    """side of the BEV logits: sparse2super's H = int(2B / voxel) (minkunet_bev.py:184-185) through MaxPool2d(5, 3, 1)
    and the two stride-2 convolutions of Encoder2D: 167 for B = 50 (bev_img_sizes, semantickitti.yaml:8), 100 for 30"""
    h = int(2 * bound_2d / voxel)
    h = (h + 2 * pool[2] - pool[0]) // pool[1] + 1
    for _ in range(2):
        h = (h + 2 - 3) // 2 + 1
    return h


def build_model(kind="MinkUNet34BEV", bound_2d=50.0, in_channels=1, out_channels=7, conv1_kernel_size=5,
                decoder_2d_levels=("block8",), device="cuda", mixstyle_layers=(), mixstyle_p=0.5, mixstyle_alpha=0.1,
                mixstyle_seed=0):
    """get_model of train_lidog.py:42-75 (MinkUNet34BEV) / train_source.py:43-58 (MinkUNet34, MinkUNet34IBN,
    MinkUNet34Robust).  `mixstyle_layers`: the encoder stages (block1 .. block4) whose output passes through a
    MinkowskiMixStyle(mixstyle_p, mixstyle_alpha) in training mode; the default builds exactly the reference's model."""
    import lidog_amd
    ms = {}
    if check_mixstyle_arguments(mixstyle_layers, mixstyle_p, mixstyle_alpha):
        ms = dict(mixstyle_layers=tuple(mixstyle_layers), mixstyle_p=mixstyle_p, mixstyle_alpha=mixstyle_alpha,
                  mixstyle_seed=mixstyle_seed)
    if kind == "MinkUNet34BEV":
        m = lidog_amd.MinkUNet34BEV(in_channels=in_channels, out_channels=out_channels, D=3,
                                    initial_kernel_size=conv1_kernel_size, decoder_2d_level=list(decoder_2d_levels),
                                    mapping_bound_2d=bound_2d, **ms)
    elif kind == "MinkUNet34":
        m = lidog_amd.MinkUNet34(in_channels=in_channels, out_channels=out_channels, D=3,
                                 initial_kernel_size=conv1_kernel_size, **ms)
    elif kind == "MinkUNet34IBN":   # train_source.py:49-53; ResNetBase drops the kernel size: conv0p1s1 is 5^3
        m = lidog_amd.MinkUNet34IBN(in_channels=in_channels, out_channels=out_channels, D=3, **ms)
    elif kind == "MinkUNet34Robust":   # the same: conv0p1s1 is 5^3
        m = lidog_amd.MinkUNet34Robust(in_channels=in_channels, out_channels=out_channels, D=3, **ms)
    else:
        raise NotImplementedError(kind)
    return m.to(device)


def mixstyle_stages_of(model):
    """the stages of `model` that carry a MinkowskiMixStyle, in stage order (() for a plain model)"""
    mods = getattr(model, "_modules", {}).get("mixstyle")
    return tuple(mods.keys()) if mods is not None else ()


def check_mixstyle(mixstyle, mixstyle_p=0.5, mixstyle_alpha=0.1, precision=None, sam_rho=None, batch_size=None,
                   what="mixstyle"):
    """The argument checks of MixStyle training (data.check_mixstyle_arguments) and what is not built: more than one
    rank, bf16 training steps, SAM (its second pass would need the first pass's draws replayed) and a batch of one scan
    (nothing to mix with).  `mixstyle`: None (off) or the stage names.  Returns the stages as a tuple."""
    if mixstyle is None:
        return ()
    layers = check_mixstyle_arguments(mixstyle, mixstyle_p, mixstyle_alpha)
    if not layers:
        raise ValueError(f"{what}: no stage named (block1 .. block4); leave it out to train without MixStyle")
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        raise NotImplementedError(f"{what} with {dist.get_world_size()} ranks: a MixStyle step leaves the trunk executor "
                                  "for the operator path and mixes within one rank's batch; data-parallel runs are "
                                  "not built")
    if _precision.resolve(precision):
        raise NotImplementedError(f"{what} with precision='bf16': MixStyle is validated on the fp32 step only")
    if sam_rho is not None:
        raise NotImplementedError(f"{what} with sam_rho: SAM's second pass would need the first pass's draws replayed")
    if batch_size is not None and batch_size < 2:
        raise ValueError(f"{what} with a batch of {batch_size} scan: a scan is mixed with another scan of its batch")
    return layers


def build_step(model, kind="MinkUNet34BEV", optimizer="Adam", lr=1e-3, scheduler=None, weight_decay=1e-4,
               momentum=0.98, warmup_epochs=0, source_weights=(0.5, 0.5), num_classes=7, ignore_label=-1, num_sources=1,
               precision=None, sem_criterion="SoftDICELoss", sem_bev_criterion=None, sem_aux_criterion=None,
               sem_aux_weight=1.0, sam_rho=None, sam_adaptive=False, grad_clip_norm=None, mixstyle=None, mixstyle_p=0.5,
               mixstyle_alpha=0.1):
    """SyncBN conversion when data-parallel (train_lidog.py:227-231), optimiser + scheduler
    (trainer_lighting_2d.py:349-394), step object (PLTTrainer2D / PLTRobustNet / PLTTrainer, on one or two sources).
    `precision`: the training steps' (trainer._Step).  `sem_criterion` / `sem_bev_criterion`: the point and BEV losses by
    name (losses.make_criterion / make_bev_criterion); the BEV one (None: DICELoss) belongs to MinkUNet34BEV alone.
    `sem_aux_criterion` (None: none) / `sem_aux_weight`: the auxiliary point loss by name (losses.make_aux_criterion) that
    every step adds to its point loss, and its weight.
    `sam_rho` (None: off) / `sam_adaptive`: sharpness-aware minimisation around the optimiser (optim.SAM: radius, the
    adaptive form); `grad_clip_norm` (None: off): the largest 2-norm of the whole gradient (trainer._Step).  One rank.
    `mixstyle` (None: the stages `model` was built with, build_model's mixstyle_layers) / `mixstyle_p` /
    `mixstyle_alpha`: checked against what MixStyle training does not support (check_mixstyle); the modules themselves
    belong to the model.
    Returns (model, step, scheduler)."""
    if num_sources not in (1, 2):
        raise NotImplementedError(f"{num_sources} sources (the reference takes one or two)")
    if sem_bev_criterion is not None and kind != "MinkUNet34BEV":
        raise ValueError(f"sem_bev_criterion={sem_bev_criterion!r}: {kind} has no BEV head")
    if _precision.resolve(precision):
        _precision.check_single_rank()
    check_sam_arguments(sam_rho, sam_adaptive, grad_clip_norm)
    if sam_rho is not None or grad_clip_norm is not None:
        _optim.check_single_rank("sam_rho / grad_clip_norm")
    if mixstyle is None and mixstyle_stages_of(model):
        mixstyle = mixstyle_stages_of(model)
    if check_mixstyle(mixstyle, mixstyle_p, mixstyle_alpha, precision, sam_rho) and \
            set(mixstyle) != set(mixstyle_stages_of(model)):
        raise ValueError(f"mixstyle={list(mixstyle)}: the model was built with {list(mixstyle_stages_of(model))} "
                         "(build_model's mixstyle_layers)")
    model = setup_data_parallel(model)
    model.train()
    opt = make_optimizer(optimizer, model, lr, weight_decay=weight_decay, momentum=momentum)
    sched = make_scheduler(scheduler, opt)
    kw = dict(source_weights=source_weights, ignore_label=ignore_label, num_sources=num_sources, precision=precision,
              sem_criterion=sem_criterion, num_classes=num_classes, sem_aux_criterion=sem_aux_criterion,
              sem_aux_weight=sem_aux_weight)
    if sam_rho is not None:
        kw["sam"] = SAM(opt, sam_rho, sam_adaptive)
    if grad_clip_norm is not None:
        kw["grad_clip_norm"] = grad_clip_norm
    if kind == "MinkUNet34BEV":
        step = LiDOGStep(model, opt, warmup_epochs=warmup_epochs, sem_bev_criterion=sem_bev_criterion or "DICELoss", **kw)
    elif kind == "MinkUNet34Robust":
        step = RobustStep(model, opt, **kw)
    else:
        step = SourceStep(model, opt, **kw)
    return model, step, sched


def _rank_world():
    if dist.is_available() and dist.is_initialized():
        return dist.get_rank(), dist.get_world_size()
    return 0, 1


def last_checkpoint(save_dir):
    """--auto_resume of train_lidog.py:142-172: the checkpoint with the highest epoch under save_dir/checkpoints"""
    d = os.path.join(save_dir, "checkpoints")
    best = None
    if os.path.isdir(d):
        for f in os.listdir(d):
            m = re.match(r"epoch=(\d+)-step=(\d+)\.ckpt$", f)
            if m and (best is None or int(m.group(1)) > best[0]):
                best = (int(m.group(1)), os.path.join(d, f))
    return best[1] if best else None


class Fit:
    """trainer.fit(pl_module, train_dataloaders, val_dataloaders, ckpt_path) of train_lidog.py:286-301."""

    def __init__(self, model_kind="MinkUNet34BEV", bound_2d=50.0, batch_size=4, optimizer="Adam", lr=1e-3,
                 scheduler=None, epochs=25, warmup_epochs=0, source_weights=(0.5, 0.5), weight_decay=1e-4,
                 momentum=0.98, check_val_every_n_epoch=5, num_sanity_val_steps=2, save_dir=None, seed=1234,
                 train_data=None, val_data=None, shuffle=True, resume=None, auto_resume=False, prefetch=True,
                 device="cuda", log=None, state_dict=None, num_sources=None, log_every_n_steps=0, metric_sources=None,
                 val_precision=None, precision=None, sem_criterion="SoftDICELoss", sem_bev_criterion=None,
                 sem_aux_criterion=None, sem_aux_weight=1.0, weight_average=None, avg_decay=0.996, avg_decay_final=None,
                 avg_start_epoch=0, sam_rho=None, sam_adaptive=False, grad_clip_norm=None, mixstyle=None, mixstyle_p=0.5,
                 mixstyle_alpha=0.1):
        """`mixstyle` (None: off; else the encoder stages, e.g. ("block1", "block2")) / `mixstyle_p` / `mixstyle_alpha`:
        MixStyle (me.MinkowskiMixStyle, include/lidog_amd.h) behind those stages in training mode: per step and stage,
        with probability p, every scan's feature statistics are mixed with another scan's of the same source's batch.
        The modules draw from their own random states, seeded from `seed`; the data pipeline's sequence is untouched.
        Validation and eval_target see the plain model; checkpoints record the three values under `mixstyle`.  One
        rank, fp32 steps, no SAM, at least two scans per batch (check_mixstyle).
        `sam_rho` / `sam_adaptive` / `grad_clip_norm`: build_step's (optim.SAM around the optimiser; the global
        gradient-norm clip).  SAM keeps no state: a resumed run passes the arguments again.
        `weight_average`: None, "ema" or "swa": an optim.WeightAverage of the model's weights and running statistics,
        updated by one launch after every training step of an epoch >= `avg_start_epoch`.  "ema" decays by `avg_decay`,
        or from `avg_decay` to `avg_decay_final` on the reference's cosine schedule over the steps that remain from
        `avg_start_epoch` to `epochs`.  Once it has been updated every validation runs a second time with the averaged
        model in place (history record `validation_avg`, metrics.jsonl keys `validation_avg/...`) and every checkpoint
        carries the average (checkpoint.save_lightning_checkpoint).  The live run does not change by a bit.
        `sem_criterion` / `sem_bev_criterion`: losses.sem_criterion / sem_bev_criterion of the reference's
        configurations, by name (build_step); the validation loss is the point criterion's.
        `sem_aux_criterion` / `sem_aux_weight`: an auxiliary point loss by name (losses.make_aux_criterion:
        LovaszSoftmaxLoss) added to the point loss times its weight, in the training steps and in the validation loss.
        `precision`: None / "fp32" (the fp32 step, exactly what runs without it) or "bf16": mixed-precision training
        steps (lidog_amd.precision: bf16 operands in the eligible sparse convolutions' forward, data-gradient and
        weight-gradient kernels, everything else -- master weights, gradients, optimiser state, checkpoints -- fp32; the
        step runs on the operator path, not the trunk executor; one rank only).  Independent of `val_precision`.
        `train_data` with `num_sources = 2` (MultiSynthScans) trains on two sources; `val_data` may then be a dict
        {source name: dataset}: every source is validated on its own (the list of loaders of train_lidog.py:186-190),
        the results keyed by name.
        `val_precision`: None / "fp32" / "bf16" (lidog_amd.precision): the validation passes' convolutions; a bf16 pass
        packs the weights once, when it starts.  It does not touch the training steps.
        `log_every_n_steps` N > 0 (the reference's entry scripts: 50): every step whose number is a multiple of N is
        recorded by a metrics.StepMetrics (per-class IoU and occurrences of the point predictions and of every BEV level,
        losses, lr; nothing is launched on the other steps), read at the end of every epoch into the history record's
        `metrics` and, with `save_dir`, appended by rank 0 to <save_dir>/metrics.jsonl together with the validation
        results.  0: off.  `metric_sources`: the source names of the keys (default: training_source_names)"""
        if _precision.resolve(precision):       # before anything is built
            _precision.check_single_rank("Fit(precision='bf16')")
        check_sam_arguments(sam_rho, sam_adaptive, grad_clip_norm)
        if sam_rho is not None or grad_clip_norm is not None:
            _optim.check_single_rank("Fit(sam_rho / grad_clip_norm)")
        self.mixstyle = check_mixstyle(mixstyle, mixstyle_p, mixstyle_alpha, precision, sam_rho, batch_size,
                                       "Fit(mixstyle)")
        self.mixstyle_p, self.mixstyle_alpha = mixstyle_p, mixstyle_alpha
        self.rank, self.world = _rank_world()
        _precision.resolve(val_precision)
        self.val_precision, self.precision = val_precision, precision
        self.kind, self.batch_size, self.epochs = model_kind, batch_size, epochs
        self.check_val, self.sanity = check_val_every_n_epoch, num_sanity_val_steps
        self.save_dir, self.seed, self.shuffle, self.prefetch = save_dir, seed, shuffle, prefetch
        self.train_data = train_data if train_data is not None else SynthScans(16)
        self.val_data = val_data
        self.device = device
        self.log = log if log is not None else (print if self.rank == 0 else (lambda *_: None))
        torch.manual_seed(seed)                         # pipeline.seed (semantickitti.yaml:32)
        model = build_model(model_kind, bound_2d, device=device, mixstyle_layers=self.mixstyle, mixstyle_p=mixstyle_p,
                            mixstyle_alpha=mixstyle_alpha, mixstyle_seed=seed)
        if state_dict is not None:
            model.load_state_dict(state_dict)
        if num_sources is None:
            num_sources = getattr(self.train_data, "num_sources", 1)
        self.model, self.step, self.sched = build_step(
            model, model_kind, optimizer, lr, scheduler, weight_decay, momentum, warmup_epochs, source_weights,
            num_sources=num_sources, precision=precision, sem_criterion=sem_criterion,
            sem_bev_criterion=sem_bev_criterion, sem_aux_criterion=sem_aux_criterion, sem_aux_weight=sem_aux_weight,
            sam_rho=sam_rho, sam_adaptive=sam_adaptive, grad_clip_norm=grad_clip_norm,
            mixstyle=self.mixstyle or None, mixstyle_p=mixstyle_p, mixstyle_alpha=mixstyle_alpha)
        self.opt = self.step.opt
        self.avg, self.avg_start_epoch = None, int(avg_start_epoch)
        if weight_average is not None:
            if not 0 <= self.avg_start_epoch < max(epochs, 1):
                raise ValueError(f"avg_start_epoch {avg_start_epoch}: an epoch of the run, 0 .. {epochs - 1}")
            per_epoch = len(self._epoch_batches(self.train_data, 0, False))
            self.avg = WeightAverage(self.opt, self.model, weight_average, avg_decay, avg_decay_final,
                                     max(per_epoch * (epochs - self.avg_start_epoch), 1))
        self.epoch, self.global_step = 0, 0
        self.history = []
        self.log_every, self.metrics, self.metrics_writer = int(log_every_n_steps), None, None
        if self.log_every > 0:
            if save_dir and self.rank == 0:
                self.metrics_writer = MetricsWriter(os.path.join(save_dir, "metrics.jsonl"))
            names = metric_sources or training_source_names(self.train_data, num_sources)
            layout = MetricLayout.for_step(self.step, names, levels=tuple(getattr(self.model, "encoders2d", {}).keys()))
            self.metrics = StepMetrics(layout, self.log_every, device=device, writer=self.metrics_writer)
        if auto_resume and save_dir and resume is None:
            resume = last_checkpoint(save_dir)
        if resume:
            ck = load_training_checkpoint(self.model, resume, self.opt, self.sched, map_location=device,
                                          weight_average=self.avg)
            self.epoch, self.global_step = ck["epoch"] + 1, ck["global_step"]
            self.log(f"resumed from {resume}: next epoch {self.epoch}, global step {self.global_step}")
            if self.avg is not None:
                self.log(f"weight average ({self.avg.mode}): {self.avg.num_updates} updates restored" if self.avg.num_updates
                         else f"weight average ({self.avg.mode}): {resume} holds none, the average starts afresh")

    # ------------------------------------------------------------------ data
    def _epoch_batches(self, data, epoch, shuffle):
        idx = shard_indices(len(data), self.rank, self.world, shuffle=shuffle, seed=self.seed, epoch=epoch)
        return [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]

    # ------------------------------------------------------------------ validation (validation_step, :295-328)
    @torch.no_grad()
    def validation_step(self, batch):
        was = self.model.training
        self.model.eval()
        st = ME.SparseTensor(coordinates=batch["coords_int"], features=batch["source_features0"])
        out = self.model(st)
        logits = (out[0] if isinstance(out, tuple) else out).F
        labels = batch["source_sem_labels0"].long()
        loss = self.step.point_loss(logits, labels)
        iou = per_class_iou(logits.max(dim=1)[1], labels)      # sklearn jaccard_score(labels=0..C-1), -1 = absent
        self.model.train(was)
        present = iou >= 0
        return {"sem_loss": float(loss), "source_iou": float(iou[present].mean()) if bool(present.any()) else 0.0,
                "per_class_iou": iou.tolist()}

    def validate(self, epoch, limit=None, tag="validation"):
        if self.val_data is None:
            return None
        if isinstance(self.val_data, dict):    # one validation set per source (validation_step's dataloader_idx)
            return {name: self._validate(data, epoch, limit, name, tag) for name, data in self.val_data.items()}
        return self._validate(self.val_data, epoch, limit, tag=tag)

    def validate_averaged(self, epoch, limit=None):
        """the same passes with the averaged weights and running statistics in place (None before the first update);
        applied() is entered outside the precision scope, so a bf16 pass packs the averaged weights"""
        if self.avg is None or self.avg.num_updates == 0 or self.val_data is None:
            return None
        with self.avg.applied():
            return self.validate(epoch, limit, tag="validation_avg")

    def _validate(self, data, epoch, limit=None, phase=None, tag="validation"):
        res = []
        with _precision.scope(self.model, self.val_precision):     # bf16: one pack per validation pass
            for ids in self._epoch_batches(data, 0, False)[:limit]:
                res.append(self.validation_step(data.batch(ids, self.device)))
        if not res:
            return None
        out = {"epoch": epoch, "sem_loss": sum(r["sem_loss"] for r in res) / len(res),
               "source_iou": sum(r["source_iou"] for r in res) / len(res), "steps": len(res)}
        if self.world > 1:   # sync_dist=True of log_losses (trainer_lighting_2d.py:330-347): mean over ranks
            t = torch.tensor([out["sem_loss"], out["source_iou"]], device=self.device, dtype=torch.float64)
            dist.all_reduce(t)
            out["sem_loss"], out["source_iou"] = (t / self.world).tolist()
        if self.metrics_writer is not None and epoch >= 0:       # not the sanity steps: Lightning logs none of them
            self.metrics_writer.write(self._validation_record(out, res, phase, tag))
        return out

    def _validation_record(self, out, res, phase, tag="validation"):
        """validation_step's keys (trainer_lighting_2d.py:316-324); a class's IoU is the mean over the batches whose
        labels hold it (on this rank), filed under its own name.  `tag`: "validation_avg" for the averaged model's pass"""
        if phase is None:
            phase = training_source_names(self.train_data, 1)[0]
        rec = {"step": self.global_step, f"{tag}/{phase}/sem_loss": out["sem_loss"],
               f"{tag}/{phase}/source_iou": out["source_iou"]}
        for c, name in enumerate(CLASS_NAMES):
            v = [r["per_class_iou"][c] for r in res if r["per_class_iou"][c] >= 0]
            if v:
                rec[f"{tag}/{phase}/{name}_source_iou"] = sum(v) / len(v)
        rec[f"{tag}/epoch"] = out["epoch"]
        return rec

    # ------------------------------------------------------------------ checkpoints (ModelCheckpoint, :222-225)
    def save(self, epoch):
        if self.save_dir is None or self.rank != 0:
            return None
        d = os.path.join(self.save_dir, "checkpoints")
        os.makedirs(d, exist_ok=True)
        path = os.path.join(d, f"epoch={epoch}-step={self.global_step}.ckpt")
        save_lightning_checkpoint(self.model, path, epoch=epoch, global_step=self.global_step, optimizer=self.opt,
                                  scheduler=self.sched, weight_average=self.avg,
                                  mixstyle={"layers": list(self.mixstyle), "p": self.mixstyle_p,
                                            "alpha": self.mixstyle_alpha} if self.mixstyle else None)
        return path

    # ------------------------------------------------------------------ the loop
    def run(self):
        if self.val_data is not None and self.sanity > 0 and self.epoch == 0:
            s = self.validate(-1, limit=self.sanity)            # num_sanity_val_steps=2 (train_lidog.py:294)
            self.log(f"sanity validation: {s}")
        for epoch in range(self.epoch, self.epochs):
            if hasattr(self.train_data, "set_epoch"):
                self.train_data.set_epoch(epoch)
            batches = self._epoch_batches(self.train_data, epoch, self.shuffle)
            cur = self.train_data.batch(batches[0], self.device) if batches else None
            losses = []
            for i in range(len(batches)):
                nxt = self.train_data.batch(batches[i + 1], self.device) if i + 1 < len(batches) else None
                if self.metrics is not None:                    # only the logged steps are recorded
                    due = (self.global_step + 1) % self.log_every == 0
                    self.step.metrics = self.metrics if due else None
                    self.metrics.next_step, self.metrics.epoch = self.global_step + 1, epoch
                out = self.step.training_step(cur, epoch=epoch, prefetch=nxt if self.prefetch else None)
                losses.append(out["loss"])
                if self.avg is not None and epoch >= self.avg_start_epoch:
                    self.avg.update()
                self.global_step += 1
                cur = nxt
            lr_used = self.opt.lr
            if self.sched is not None:
                self.sched.step()                               # interval='epoch'
            rec = {"epoch": epoch, "global_step": self.global_step, "lr": lr_used,
                   "loss": float(torch.stack(losses).mean()) if losses else float("nan"),
                   "losses": [float(l) for l in losses]}
            if self.metrics is not None:
                rec["metrics"] = self.metrics.finish()
            if self.val_data is not None and (epoch + 1) % self.check_val == 0:
                rec["validation"] = self.validate(epoch)
                if self.avg is not None and self.avg.num_updates > 0:
                    rec["validation_avg"] = self.validate_averaged(epoch)
            if dist.is_available() and dist.is_initialized():
                from .comm import _TRANSPORTS
                for tr in _TRANSPORTS.values():                 # a statistics message that never arrived invalidates the epoch
                    tr.check()
            rec["checkpoint"] = self.save(epoch)                # every_n_epochs=1, save_top_k=-1
            self.history.append(rec)
            self.log({k: v for k, v in rec.items() if k != "losses"})
            self.epoch = epoch + 1
        if self.metrics is not None:
            self.metrics.finish()
        if self.world > 1:
            dist.barrier()
        return self.history


Trainer = Fit


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--model", default="MinkUNet34BEV", choices=["MinkUNet34BEV", "MinkUNet34", "MinkUNet34IBN",
                                                                    "MinkUNet34Robust"])
    ap.add_argument("--bound", type=float, default=50.0)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--optimizer", default="Adam", choices=["Adam", "SGD"])
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--scheduler", default=None, choices=[None, "CosineAnnealingLR", "ExponentialLR", "CyclicLR"])
    ap.add_argument("--epochs", type=int, default=25)
    ap.add_argument("--warmup-epochs", type=int, default=0)
    ap.add_argument("--scans", type=int, default=16, help="synthetic training scans per epoch (all ranks together)")
    ap.add_argument("--val-scans", type=int, default=0)
    ap.add_argument("--config", default=None, choices=sorted(synth.CONFIGS), help="default: kitti120k")
    ap.add_argument("--sources", nargs=2, default=None, choices=sorted(synth.CONFIGS), metavar="CONFIG",
                    help="train on two sources (configs/*/multi/*.yaml): --scans scans of each, paired as "
                         "MultiBEVSourceDataset; each source is validated on its own")
    ap.add_argument("--source-weights", nargs=2, type=float, default=(0.5, 0.5))
    ap.add_argument("--mix3d", action="store_true")
    ap.add_argument("--mix", default=None, choices=MixedSynthScans.METHODS + MixedSynthScans.SENSOR_METHODS,
                    help="PointCutMix / CoSMix (train_aug_based.py, pipeline.method): each item one scan mixed from a "
                         "pair of the two --sources (default: --config twice), trained as one source with SoftDICE; "
                         "polarmix / lasermix: the sensor-aware mixes (an azimuth sector swapped and instance classes "
                         "pasted rotated; the scans interleaved by inclination band), used the same way")
    ap.add_argument("--sub-p", type=float, default=0.8, help="CoSMix: share of each drawn class's rows mixed in; "
                                                             "--augment: the datasets' sub_p, the share of a scan's "
                                                             "points every item draws")
    ap.add_argument("--augment", nargs="*", default=None, metavar="NAME",
                    help="the training datasets' augmentation_list: any ordered list of RandomRotation and RandomScale "
                         "(the empty list: sub-sampling only).  Every item is then made from the scan's points on the "
                         "GPU: --sub-p of them in random order, transformed, voxelised; MinkUNet34BEV also gets the "
                         "bounds filter and BEV labels rasterised from the item")
    ap.add_argument("--sn-targets", nargs="+", default=None, choices=sorted(synth.CONFIGS), metavar="CONFIG",
                    help="SN car-size scaling (train_scaling_based.py): every scan of --config (or of the two --sources) "
                         "is scaled to the car size of these target configurations and re-quantised; the car sizes "
                         "are clustered on the GPU at start-up; trained with SoftDICE (use the *_cars configurations)")
    ap.add_argument("--raycast-to", default=argparse.SUPPRESS, metavar="NAME|FILE.json",
                    help="the Raycast baseline (configs/raycast): every training scan is resampled on the GPU as the "
                         "target's sensor would have recorded it (lidog_amd.raycast): a configuration's sensor, hdl32e, "
                         "or a JSON file; --augment runs after the resampling; validation data is never resampled")
    ap.add_argument("--raycast-origin", nargs=3, type=float, default=argparse.SUPPRESS, metavar=("X", "Y", "Z"),
                    help="the target sensor's position in the source frame (default: the height difference of two "
                         "synthetic configurations, else 0 0 0)")
    ap.add_argument("--check-val-every-n-epoch", type=int, default=5)
    ap.add_argument("--save-dir", default=None)
    ap.add_argument("--resume", default=None)
    ap.add_argument("--auto-resume", action="store_true")
    ap.add_argument("--seed", type=int, default=1234)
    # the flags below have no attribute unless they are given (argparse.SUPPRESS): read them with getattr
    ap.add_argument("--source-augment", nargs="*", default=argparse.SUPPRESS, metavar="NAME",
                    help="with --mix, --mix3d, --sn-targets or --sn-target-files: the SOURCE datasets' augmentation_list "
                         "(and --sub-p their sub_p), as the reference's configs/{mix3D,pointcutmix,cosmix,SN} set it: "
                         "every item is sub-sampled, transformed and voxelised before it is mixed or scaled, CoSMix "
                         "transforms every pasted class once more, and the SN car sizes are measured on the augmented "
                         "items.  With --mix3d every item becomes one scan merged on the GPU")
    ap.add_argument("--sn-target-files", nargs="+", default=argparse.SUPPRESS, metavar="NAME=PATH",
                    help="SN over --files: the target datasets (their validation listings give the target car sizes)")
    ap.add_argument("--sn-target-label-maps", nargs="+", default=argparse.SUPPRESS, metavar="FILE",
                    help="one label map per --sn-target-files entry")
    ap.add_argument("--mix-pitch", nargs=2, type=float, default=argparse.SUPPRESS, metavar=("LO", "HI"),
                    help="--mix lasermix: the sensor's vertical field of view in degrees, cut into the inclination bands "
                         "(default -25 3)")
    ap.add_argument("--mix-instance-classes", nargs="+", type=int, default=argparse.SUPPRESS, metavar="C",
                    help="--mix polarmix: the classes whose rows are pasted rotated (default 0 1: vehicle, person)")
    ap.add_argument("--log-every-n-steps", type=int, default=argparse.SUPPRESS, metavar="N",
                    help="record per-class IoU, class counts, losses and lr of every N-th training step on the GPU and "
                         "append them to <save-dir>/metrics.jsonl (the reference's entry scripts: 50; default 0: off)")
    ap.add_argument("--val-precision", default=argparse.SUPPRESS, choices=["fp32", "bf16"],
                    help="precision of the validation passes' convolutions (default fp32; bf16: lidog_amd.precision, the "
                         "weights are packed once per validation pass); independent of --precision")
    ap.add_argument("--precision", default=argparse.SUPPRESS, choices=["fp32", "bf16"],
                    help="precision of the training steps (default fp32; bf16: the sparse convolutions with channel "
                         "counts that are multiples of 32 run forward, data gradient and weight gradient on bf16 operands "
                         "with fp32 accumulation, lidog_amd.precision; weights, gradients, optimiser state and "
                         "checkpoints stay fp32; one GPU)")
    ap.add_argument("--sem-criterion", default=argparse.SUPPRESS, choices=list(POINT_CRITERIA),
                    help="the point loss (losses.sem_criterion of the reference's configurations; default SoftDICELoss)")
    ap.add_argument("--sem-bev-criterion", default=argparse.SUPPRESS, choices=list(BEV_CRITERIA),
                    help="the BEV loss of MinkUNet34BEV (losses.sem_bev_criterion; default DICELoss)")
    ap.add_argument("--sem-aux-criterion", default=argparse.SUPPRESS, choices=list(AUX_CRITERIA),
                    help="an auxiliary point loss added to --sem-criterion's in every step and in the validation loss "
                         "(LovaszSoftmaxLoss: the mIoU surrogate of Berman et al., csrc/lovasz.hip; default: none)")
    ap.add_argument("--sem-aux-weight", type=float, default=argparse.SUPPRESS, metavar="W",
                    help="weight of --sem-aux-criterion in the point loss (default 1.0)")
    ap.add_argument("--weight-average", default=argparse.SUPPRESS, choices=list(WeightAverage.MODES),
                    help="average the weights and running statistics along the trajectory, one launch per step "
                         "(optim.WeightAverage): ema (the reference's MomentumUpdater) or swa (the uniform average); "
                         "validation then also scores the averaged model and checkpoints carry it "
                         "(eval_target --weights averaged)")
    ap.add_argument("--avg-decay", type=float, default=argparse.SUPPRESS, metavar="TAU",
                    help="ema: the decay, in [0, 1] (default 0.996)")
    ap.add_argument("--avg-decay-final", type=float, default=argparse.SUPPRESS, metavar="TAU",
                    help="ema: the decay rises from --avg-decay to this on a cosine over the averaged steps "
                         "(default: constant)")
    ap.add_argument("--avg-start-epoch", type=int, default=argparse.SUPPRESS, metavar="E",
                    help="the first epoch whose steps are averaged (default 0)")
    ap.add_argument("--sam-rho", type=float, default=argparse.SUPPRESS, metavar="R",
                    help="sharpness-aware minimisation (optim.SAM): every step takes its gradient at the worst point of a "
                         "neighbourhood of radius R of the weights, at the cost of a second forward and backward pass "
                         "(usual: 0.05; with --sam-adaptive 0.5 to 2; one GPU; default: off)")
    ap.add_argument("--sam-adaptive", action="store_true", default=argparse.SUPPRESS,
                    help="--sam-rho's adaptive form (ASAM): the neighbourhood scales with every weight's magnitude")
    ap.add_argument("--grad-clip-norm", type=float, default=argparse.SUPPRESS, metavar="X",
                    help="scale the gradient so that its global 2-norm is at most X (torch's clip_grad_norm_, Lightning's "
                         "gradient_clip_val; one GPU; default: off)")
    ap.add_argument("--mixstyle", nargs="*", default=argparse.SUPPRESS, metavar="STAGE",
                    help="MixStyle (Zhou et al., ICLR 2021; csrc/mixstyle.hip): in training, every scan's per-channel "
                         "feature mean and standard deviation behind these encoder stages (block1 .. block4; the bare "
                         "flag: block1 block2) are interpolated with another scan's of the batch; validation and "
                         "evaluation see the plain model (one GPU, fp32, not with --sam-rho, --batch >= 2; default: off)")
    ap.add_argument("--mixstyle-p", type=float, default=argparse.SUPPRESS, metavar="P",
                    help="--mixstyle: the probability that a stage mixes in a step (default 0.5)")
    ap.add_argument("--mixstyle-alpha", type=float, default=argparse.SUPPRESS, metavar="A",
                    help="--mixstyle: the mixing weights are drawn from Beta(A, A) per scan (default 0.1)")
    scans.add_file_arguments(ap, "--files", "train on")
    a = ap.parse_args(argv)
    if hasattr(a, "mixstyle"):
        if not a.mixstyle:
            a.mixstyle = list(MIXSTYLE_DEFAULT_STAGES)
        try:
            check_mixstyle(a.mixstyle, getattr(a, "mixstyle_p", 0.5), getattr(a, "mixstyle_alpha", 0.1),
                           getattr(a, "precision", None), getattr(a, "sam_rho", None), a.batch, "--mixstyle")
        except (ValueError, NotImplementedError) as e:
            ap.error(str(e))
    else:
        for name in ("mixstyle_p", "mixstyle_alpha"):
            if hasattr(a, name):
                ap.error(f"--{name.replace('_', '-')} goes with --mixstyle")
    try:
        check_sam_arguments(**sam_of(a))
    except ValueError as e:
        ap.error(str(e))
    if not hasattr(a, "weight_average"):
        for name in ("avg_decay", "avg_decay_final", "avg_start_epoch"):
            if hasattr(a, name):
                ap.error(f"--{name.replace('_', '-')} goes with --weight-average")
    else:
        try:
            WeightAverage.check_arguments(a.weight_average, getattr(a, "avg_decay", 0.996),
                                          getattr(a, "avg_decay_final", None), 1)
        except ValueError as e:
            ap.error(f"--weight-average: {e}")
        if not 0 <= getattr(a, "avg_start_epoch", 0) < max(a.epochs, 1):
            ap.error(f"--avg-start-epoch {a.avg_start_epoch}: an epoch of the run, 0 .. {a.epochs - 1}")
    if hasattr(a, "sem_aux_weight") and not hasattr(a, "sem_aux_criterion"):
        ap.error("--sem-aux-weight goes with --sem-aux-criterion")
    if hasattr(a, "sem_aux_weight") and not a.sem_aux_weight > 0:
        ap.error(f"--sem-aux-weight {a.sem_aux_weight}: the weight is positive")
    if getattr(a, "sem_bev_criterion", None) is not None and a.model != "MinkUNet34BEV":
        ap.error(f"--sem-bev-criterion is the loss of the BEV head: --model MinkUNet34BEV, not {a.model}")
    source_augment = getattr(a, "source_augment", None)
    sn_target_files = getattr(a, "sn_target_files", None)
    sn_target_label_maps = getattr(a, "sn_target_label_maps", None)
    if a.files is not None:
        for flag, given in (("--config", a.config is not None), ("--sources", a.sources is not None)):
            if given:
                ap.error(f"--files with {flag}: scans come either from files or from the synthetic generator")
        if a.sn_targets is not None:
            ap.error("--files with --sn-targets: the targets of SN over files are files too, pass --sn-target-files "
                     "NAME=PATH ... with --sn-target-label-maps")
        if (a.mix is not None or a.mix3d) and len(a.files) != 2:
            ap.error(f"--files with {'--mix' if a.mix is not None else '--mix3d'}: a mix pairs two datasets, pass exactly "
                     f"two entries A=PATH B=PATH")
        a.files = scans.check_file_arguments(ap, a.files, a, "--files")
    elif a.label_maps is not None or a.synth4d_splits is not None or a.limit_files is not None:
        ap.error("--label-maps, --synth4d-splits and --limit-files go with --files")
    if sn_target_files is not None:
        if a.files is None:
            ap.error("--sn-target-files goes with --files (synthetic scans take --sn-targets)")
        try:
            a.sn_target_files = sn_target_files = scans.parse_files(sn_target_files)
        except ValueError as e:
            ap.error(f"--sn-target-files: {e}")
        if sn_target_label_maps is None or len(sn_target_label_maps) != len(sn_target_files):
            ap.error("--sn-target-files needs --sn-target-label-maps with one file per entry")
        if any("Synth4D" in n for n, _ in sn_target_files) and a.synth4d_splits is None:
            ap.error("--sn-target-files: a Synth4D entry needs --synth4d-splits")
    elif sn_target_label_maps is not None:
        ap.error("--sn-target-label-maps goes with --sn-target-files")
    sn = a.sn_targets is not None or sn_target_files is not None
    if source_augment is not None:
        check_augmentations(source_augment)       # NotImplementedError for another name, as get_augmentations
        if a.augment is not None:
            ap.error("--source-augment with --augment: --augment is a plain training dataset's list, --source-augment "
                     "the list of the source datasets under a mixing or SN dataset; pass one of them")
        if not (a.mix is not None or a.mix3d or sn):
            ap.error("--source-augment goes with --mix, --mix3d, --sn-targets or --sn-target-files (a plain training "
                     "dataset takes --augment)")
    if a.config is None:
        a.config = "kitti120k"
    if mix_method_of(a) == "mix3d":
        if a.model in ("MinkUNet34BEV", "MinkUNet34Robust"):   # one merged scan per item, PLTMixed: SoftDICE only
            ap.error(f"--mix3d with --source-augment or --files trains on merged items with the SoftDICE-only step of "
                     f"PLTMixed: --model MinkUNet34 or MinkUNet34IBN, not {a.model}")
        if a.files is None and a.sources is None:
            a.sources = [a.config, a.config]
    if a.mix is not None:
        if a.model in ("MinkUNet34BEV", "MinkUNet34Robust"):   # PLTMixed.training_step: SoftDICE only
            ap.error(f"--mix trains with the SoftDICE-only step of PLTMixed: --model MinkUNet34 or MinkUNet34IBN, "
                     f"not {a.model}")
        if a.mix3d:
            ap.error("--mix and --mix3d are two different methods (pipeline.method): pass one of them")
        if a.sources is None and a.files is None:
            a.sources = [a.config, a.config]    # the single configs list one dataset twice
    for name, method in (("mix_pitch", "lasermix"), ("mix_instance_classes", "polarmix")):
        if hasattr(a, name) and a.mix != method:
            ap.error(f"--{name.replace('_', '-')} goes with --mix {method}")
    try:
        if hasattr(a, "mix_pitch"):
            band_bounds(a.mix_pitch, 1)
        if hasattr(a, "mix_instance_classes"):
            instance_mask(a.mix_instance_classes)
    except ValueError as e:
        ap.error(f"--mix {a.mix}: {e}")
    if sn:
        flag = "--sn-targets" if a.sn_targets is not None else "--sn-target-files"
        if a.model in ("MinkUNet34BEV", "MinkUNet34Robust"):   # train_scaling_based.py:142-155, PLTTrainer: SoftDICE only
            ap.error(f"{flag} trains with the SoftDICE-only step of PLTTrainer: --model MinkUNet34 or "
                     f"MinkUNet34IBN, not {a.model}")
        if a.mix is not None or a.mix3d:
            ap.error(f"{flag}, --mix and --mix3d are different methods: pass one of them")
    if getattr(a, "raycast_to", None) is not None:
        if a.mix is not None or a.mix3d or sn:
            ap.error("--raycast-to, --mix, --mix3d and --sn-targets are different methods: pass one of them")
        from .raycast import sensor
        try:
            sensor(a.raycast_to)
        except ValueError as e:
            ap.error(f"--raycast-to: {e}")
    elif getattr(a, "raycast_origin", None) is not None:
        ap.error("--raycast-origin goes with --raycast-to")
    if a.augment is not None:
        check_augmentations(a.augment)       # NotImplementedError for another name, as get_augmentations
        if a.mix is not None or a.mix3d or sn:
            ap.error("--augment with --mix, --mix3d or --sn-targets: under those datasets the list belongs to the SOURCE "
                     "datasets and is applied to the items and again inside CoSMix's merge: pass --source-augment")
    return a


def mix_method_of(a):
    """the method of MixedSynthScans the arguments ask for, or None: --mix M; --mix3d once its items are merged on the
    GPU (with --source-augment or --files; plain --mix3d keeps the host-made synthetic union)"""
    if getattr(a, "mix", None) is not None:
        return a.mix
    merged = getattr(a, "source_augment", None) is not None or getattr(a, "files", None) is not None
    return "mix3d" if getattr(a, "mix3d", False) and merged else None


def mix_options_of(a):
    """MixedSynthScans' pitch / instance_classes of parsed arguments (its defaults when the flags were not given)"""
    kw = {}
    if getattr(a, "mix_pitch", None) is not None:
        kw["pitch"] = tuple(a.mix_pitch)
    if getattr(a, "mix_instance_classes", None) is not None:
        kw["instance_classes"] = tuple(a.mix_instance_classes)
    return kw


def val_precision_of(a):
    """--val-precision of parsed arguments ("fp32" when it was not given)"""
    return getattr(a, "val_precision", "fp32")


def precision_of(a):
    """--precision of parsed arguments (None, the fp32 step as it always ran, when it was not given)"""
    return getattr(a, "precision", None)


def sem_criterion_of(a):
    """--sem-criterion of parsed arguments ("SoftDICELoss" when it was not given)"""
    return getattr(a, "sem_criterion", "SoftDICELoss")


def sem_bev_criterion_of(a):
    """--sem-bev-criterion of parsed arguments; not given: "DICELoss" for MinkUNet34BEV, None for a model without the
    BEV head"""
    return getattr(a, "sem_bev_criterion", "DICELoss" if a.model == "MinkUNet34BEV" else None)


def sem_aux_of(a):
    """(--sem-aux-criterion, --sem-aux-weight) of parsed arguments: (None, 1.0) when they were not given"""
    return getattr(a, "sem_aux_criterion", None), getattr(a, "sem_aux_weight", 1.0)


def sam_of(a):
    """build_step's sam_rho / sam_adaptive / grad_clip_norm of parsed arguments (off when they were not given)"""
    return dict(sam_rho=getattr(a, "sam_rho", None), sam_adaptive=getattr(a, "sam_adaptive", False),
                grad_clip_norm=getattr(a, "grad_clip_norm", None))


def mixstyle_of(a):
    """Fit's mixstyle / mixstyle_p / mixstyle_alpha of parsed arguments (mixstyle None when the flag was not given)"""
    return dict(mixstyle=getattr(a, "mixstyle", None), mixstyle_p=getattr(a, "mixstyle_p", 0.5),
                mixstyle_alpha=getattr(a, "mixstyle_alpha", 0.1))


def weight_average_of(a):
    """Fit's weight_average / avg_* arguments of parsed arguments (weight_average None when it was not given)"""
    return dict(weight_average=getattr(a, "weight_average", None), avg_decay=getattr(a, "avg_decay", 0.996),
                avg_decay_final=getattr(a, "avg_decay_final", None), avg_start_epoch=getattr(a, "avg_start_epoch", 0))


def main(argv=None):
    a = parse_args(argv)
    fit = _fit_from_args(a)
    fit.run()
    _finish_distributed()


def _fit_from_args(a):
    """the Fit of parsed command-line arguments (process group set up when launched as several ranks)"""
    world = int(os.environ.get("WORLD_SIZE", 1))
    local = int(os.environ.get("LOCAL_RANK", 0))
    torch.cuda.set_device(local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    train, val = _data_from_args(a)
    sem_aux_criterion, sem_aux_weight = sem_aux_of(a)
    return Fit(a.model, a.bound, a.batch, a.optimizer, a.lr, a.scheduler, a.epochs, a.warmup_epochs,
               source_weights=tuple(a.source_weights), check_val_every_n_epoch=a.check_val_every_n_epoch,
               save_dir=a.save_dir, seed=a.seed, train_data=train, val_data=val, resume=a.resume,
               auto_resume=a.auto_resume, log_every_n_steps=getattr(a, "log_every_n_steps", 0),
               val_precision=val_precision_of(a), precision=precision_of(a), sem_criterion=sem_criterion_of(a),
               sem_bev_criterion=sem_bev_criterion_of(a), sem_aux_criterion=sem_aux_criterion,
               sem_aux_weight=sem_aux_weight, **weight_average_of(a), **sam_of(a), **mixstyle_of(a))


def _data_from_args(a):
    """(training dataset, validation dataset or {name: dataset} or None) of parsed command-line arguments"""
    bev = bev_image_size(a.bound)
    src_aug = getattr(a, "source_augment", None)
    mix_method = mix_method_of(a)

    def per_source_val():                   # validation data is never augmented or mixed
        return {name: SynthScans(a.val_scans, c, first=10 ** 6 + i * synth.SOURCE1_SEED, bev_size=bev)
                for i, (name, c) in enumerate(zip(source_names(a.sources), a.sources))} if a.val_scans else None

    if getattr(a, "files", None):
        train, val = _file_data(a, bev)
    elif src_aug is not None and mix_method is not None:
        items = AugmentedSynthScans(a.scans, a.sources, src_aug, sub_p=a.sub_p, seed=a.seed)
        train = MixedSynthScans(a.scans, a.scans, a.sources, method=mix_method, seed=a.seed, items=items,
                                **mix_options_of(a))
        val = per_source_val()
    elif src_aug is not None:               # --sn-targets
        configs = a.sources or [a.config]
        items = AugmentedSynthScans(a.scans, configs, src_aug, sub_p=a.sub_p, seed=a.seed)
        train = ScaledSynthScans(a.scans, configs, a.sn_targets, seed=a.seed, items=items)
        val = per_source_val() if a.sources else (
            SynthScans(a.val_scans, a.config, first=10 ** 6, bev_size=bev) if a.val_scans else None)
    elif getattr(a, "augment", None) is not None or getattr(a, "raycast_to", None) is not None:
        train = AugmentedSynthScans(a.scans, a.sources or a.config, a.augment, sub_p=a.sub_p, seed=a.seed,
                                    bev=(a.bound, bev) if a.model == "MinkUNet34BEV" else None,
                                    raycast=getattr(a, "raycast_to", None),
                                    raycast_origin=getattr(a, "raycast_origin", None))
        if a.sources:                       # validation data is never augmented (phase == 'train' only)
            val = {name: SynthScans(a.val_scans, c, first=10 ** 6 + i * synth.SOURCE1_SEED, bev_size=bev)
                   for i, (name, c) in enumerate(zip(source_names(a.sources), a.sources))} if a.val_scans else None
        else:
            val = SynthScans(a.val_scans, a.config, first=10 ** 6, bev_size=bev) if a.val_scans else None
    elif getattr(a, "sn_targets", None):
        configs = a.sources or [a.config]
        train = ScaledSynthScans(a.scans, configs, a.sn_targets, seed=a.seed)
        if a.sources:
            val = {name: SynthScans(a.val_scans, c, first=10 ** 6 + i * synth.SOURCE1_SEED, bev_size=bev)
                   for i, (name, c) in enumerate(zip(source_names(a.sources), a.sources))} if a.val_scans else None
        else:
            val = SynthScans(a.val_scans, a.config, first=10 ** 6, bev_size=bev) if a.val_scans else None
    elif getattr(a, "mix", None):
        train = MixedSynthScans(a.scans, a.scans, a.sources, method=a.mix, sub_p=a.sub_p, seed=a.seed,
                                **mix_options_of(a))
        val = {name: SynthScans(a.val_scans, c, first=10 ** 6 + i * synth.SOURCE1_SEED, bev_size=bev)
               for i, (name, c) in enumerate(zip(source_names(a.sources), a.sources))} if a.val_scans else None
    elif a.sources:
        train = MultiSynthScans(a.scans, a.scans, a.sources, seed=a.seed, mix3d=a.mix3d, bev_size=bev)
        val = {name: SynthScans(a.val_scans, c, first=10 ** 6 + i * synth.SOURCE1_SEED, mix3d=a.mix3d, bev_size=bev)
               for i, (name, c) in enumerate(zip(source_names(a.sources), a.sources))} if a.val_scans else None
    else:
        train = SynthScans(a.scans, a.config, mix3d=a.mix3d, bev_size=bev)
        val = SynthScans(a.val_scans, a.config, first=10 ** 6, mix3d=a.mix3d, bev_size=bev) if a.val_scans else None
    return train, val


def _file_data(a, bev):
    """--files: (training dataset, {name: validation dataset}) over the listings of phase train / validation"""
    luts = scans.luts_from_files(a.label_maps)
    kw = dict(version=a.version, synth4d_splits=a.synth4d_splits, limit=a.limit_files)
    listings = [scans.listing(n, p, "train", **kw) for n, p in a.files]
    mix_method, sn_files = mix_method_of(a), getattr(a, "sn_target_files", None)
    src_aug = getattr(a, "source_augment", None)
    if mix_method is not None or sn_files:
        # the source datasets under a mixing / SN dataset: their items are what FileScans makes, with --source-augment
        items = scans.FileScans(listings, luts, augmentations=src_aug, sub_p=a.sub_p, seed=a.seed)
        names = [n for n, _ in a.files]
        if mix_method is not None:
            train = MixedSynthScans(len(listings[0]), len(listings[1]), names, method=mix_method, seed=a.seed,
                                    items=items, **mix_options_of(a))
        else:
            faces = []
            for (n, p), lut in zip(sn_files, scans.luts_from_files(a.sn_target_label_maps)):
                tgt = scans.FileScans(scans.listing(n, p, "validation", **kw), lut, seed=a.seed)
                faces.append(ItemFace(tgt, 0, len(tgt), None))
            train = ScaledSynthScans([len(l) for l in listings], names, [n for n, _ in sn_files], seed=a.seed,
                                     items=items, target_faces=faces)
    else:
        train = scans.FileScans(listings, luts, augmentations=a.augment, sub_p=a.sub_p, seed=a.seed,
                                bev=(a.bound, bev) if a.model == "MinkUNet34BEV" else None,
                                raycast=getattr(a, "raycast_to", None),
                                raycast_origin=getattr(a, "raycast_origin", None))
    val = {name: scans.FileScans(scans.listing(n, p, "validation", **kw), lut, seed=a.seed)
           for name, (n, p), lut in zip(source_names([n for n, _ in a.files]), a.files, luts)}
    return train, val


def _finish_distributed():
    world = int(os.environ.get("WORLD_SIZE", 1))
    if world > 1:
        dist.barrier()
        torch.cuda.synchronize()
        from . import comm
        comm.reset()                 # this library's RCCL communicators / mailboxes go before torch's group does
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
