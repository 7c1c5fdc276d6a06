"""Per-step training metrics: what every training pipeline of the reference logs through `log_losses`
(utils/pipelines/trainer_lighting_2d.py:203-291, trainer_lighting_2d_multi.py:217-305, trainer_lighting.py:118-153,
trainer_lighting_mix.py, trainer_lighting_SN.py, trainer_lighting_robustnet.py; log_every_n_steps=50 in every entry
script): per-class IoU and class occurrences of the point predictions of each source and of every BEV level, the
losses, the learning rate and the epoch.

The reference pays several device-to-host copies and sklearn / torchmetrics calls on the CPU per step.  Here a logged
step makes ONE launch (csrc/trainstats.hip: integer confusion counts of every tensor) into a slot of a device ring;
the ring is turned into values on the device, averaged over the ranks with one all-reduce and copied to a pinned
buffer behind an event; the host reads a buffer one flush later.  No step waits for the device.

    train_confusion   (logits, labels) pairs -> counts [segments, C + 1, C] int64 on the device, one launch
    iou_from_counts   counts -> (iou, present, occurrences), any device
    MetricLayout      the keys of a run: sources, BEV levels, losses
    StepMetrics       the ring: record() per logged step, flush() / finish()
    MetricsWriter     <save_dir>/metrics.jsonl, one JSON object per logged step

One deliberate deviation from the reference: it zips the names of the PRESENT classes with the IoU list of ALL classes,
so a value lands under the wrong name whenever a class is absent from the batch; here every value is filed under its
own class.  The means are unaffected."""
import ctypes
import json
import os

import torch
import torch.distributed as dist

from .evaluate import CLASS_NAMES, MAX_CLASSES

MAX_SEGMENTS = 8


def train_confusion(pairs, num_classes=7, ignore_label=-1, out=None, err=None):
    """counts [len(pairs), C + 1, C] int64 of lidog_train_confusion, on the device, in one launch for all pairs.
    `pairs`: 1..8 (logits, labels) device tensors; logits float32 with C * labels.numel() elements, read as contiguous
    rows of C floats (a [N, C] matrix, or a contiguous NCHW BEV tensor as `.view(b, h, w, -1)` reads it), labels int64.
    counts[s, label + 1, pred], row 0 for the ignore label and for every label outside 0..C-1; pred = the first maximal
    index (the first NaN in a row holding one).  `out`: counts to ADD to.  `err`: an int32 [1] device word in which
    bit s is set when segment s holds a label other than ignore_label outside 0..C-1, for check_label_error later
    (nothing is read back here); without it this call checks, which costs one synchronisation."""
    from ._lib import call, ptr, require_gpu
    pairs = list(pairs)
    k, c = len(pairs), int(num_classes)
    if not 1 <= k <= MAX_SEGMENTS:
        raise ValueError(f"train_confusion: {k} pairs (1..{MAX_SEGMENTS})")
    if not 1 <= c <= MAX_CLASSES:
        raise ValueError(f"train_confusion: {c} classes (1..{MAX_CLASSES})")
    lp, bp, nn = (ctypes.c_void_p * k)(), (ctypes.c_void_p * k)(), (ctypes.c_int64 * k)()
    keep = []
    dev = pairs[0][0].device
    for s, (logits, labels) in enumerate(pairs):
        require_gpu(logits, "logits")
        n = labels.numel()
        if logits.dtype != torch.float32 or logits.numel() != n * c or logits.device != dev:
            raise ValueError(f"train_confusion: pair {s}: logits must be float32 with {n} x {c} elements on {dev}, got "
                             f"{logits.dtype} {tuple(logits.shape)} on {logits.device}")
        if labels.dtype != torch.int64 or labels.device != dev:
            raise ValueError(f"train_confusion: pair {s}: labels must be int64 on {dev}, got {labels.dtype} on "
                             f"{labels.device}")
        logits, labels = logits.detach().contiguous(), labels.contiguous()
        keep.append((logits, labels))
        nn[s] = n
        lp[s], bp[s] = (logits.data_ptr(), labels.data_ptr()) if n else (None, None)
    if out is None:
        out = torch.zeros((k, c + 1, c), dtype=torch.int64, device=dev)
    elif out.shape != (k, c + 1, c) or out.dtype != torch.int64 or not out.is_contiguous() or out.device != dev:
        raise ValueError(f"train_confusion: out must be a contiguous int64 [{k}, {c + 1}, {c}] tensor on {dev}")
    own_err = err is None
    if own_err:
        err = torch.zeros(1, dtype=torch.int32, device=dev)
    call("lidog_train_confusion", lp, bp, nn, k, c, int(ignore_label), ptr(out), ptr(err))
    if own_err:
        check_label_error(err)
    return out


def check_label_error(err, what="train_confusion"):
    """raises when a segment held a label outside 0..C-1 other than the ignore label (`err`: the word or its value)"""
    bits = int(err.item()) if torch.is_tensor(err) else int(err)
    if bits:
        segs = [s for s in range(MAX_SEGMENTS) if bits >> s & 1]
        raise ValueError(f"{what}: labels outside the classes (and not the ignore label) in segment(s) {segs}; they were "
                         f"counted as ignored")


def iou_from_counts(counts, count_ignored):
    """(iou [.., C] float64, present [.., C] bool, occurrences [.., C] int64) of counts [.., C + 1, C], on the counts'
    device.  iou = intersection / union as one float64 division, 0 where the union is empty (sklearn's
    zero_division=0., torchmetrics' absent score).  count_ignored=False drops row 0: the LiDOG trainers, which filter
    label == -1 before JaccardIndex.  count_ignored=True lets an ignored row enlarge the union of the class it is
    predicted as: jaccard_score over all rows in the source / mix / SN / RobustNet trainers (evaluate.per_class_iou).
    present: the class occurs in the labels; occurrences: how often (torch.unique(labels, return_counts=True))."""
    c = counts.shape[-1]
    if counts.dim() < 2 or counts.shape[-2] != c + 1:
        raise ValueError(f"iou_from_counts: counts must be [.., C + 1, C], got {tuple(counts.shape)}")
    lab = counts[..., 1:, :]
    tp = torch.diagonal(lab, dim1=-2, dim2=-1)
    true = lab.sum(dim=-1)
    pred = (counts if count_ignored else lab).sum(dim=-2)
    union = true + pred - tp
    iou = tp.double() / union.clamp(min=1).double()         # an empty union has an empty intersection: 0 / 1
    return iou, true > 0, true


def mean_present(iou, present):
    """the logged mean: over the present classes, 0 if there are none"""
    p = present.to(iou.dtype)
    return (iou * p).sum(dim=-1) / p.sum(dim=-1).clamp(min=1)


class MetricLayout:
    """The keys of a run, the reference's.  Segments (the tensors of one launch), per source: its point logits, then
    each BEV level.  The packed vector of a step, K entries: per segment C IoU, C occurrence counts and the mean IoU;
    then the losses; then the lr.
      point segment   training/<source>/<class>_iou, .._count, training/<source>/source_iou<s>
      BEV level       training/<source>/<class>_iou_bev_<lvl>, .._count_bev_<lvl>, training/<source>/source_iou_bev<s>_<lvl>
      losses          training/<source s>/<name><s> (sem_loss, bev_loss, aux_loss), training/<source 0>/total_loss
      run             training/lr, training/epoch
    `losses`: the names of the step's loss dict ("sem_loss", or "sem_loss0", "sem_loss1" with two sources; "loss" is the
    total)."""

    def __init__(self, sources, losses=("sem_loss",), levels=(), count_ignored=True, class_names=None, num_classes=None):
        self.sources, self.losses, self.levels = tuple(sources), tuple(losses), tuple(levels)
        self.count_ignored = bool(count_ignored)
        self.class_names = tuple(CLASS_NAMES if class_names is None else class_names)
        if num_classes is not None and num_classes != len(self.class_names):
            self.class_names = tuple(f"class{i}" for i in range(num_classes))
        self.num_classes = len(self.class_names)
        self.segments = [(s, lvl) for s in range(len(self.sources)) for lvl in (None,) + self.levels]
        if not 1 <= len(self.segments) <= MAX_SEGMENTS:
            raise ValueError(f"{len(self.segments)} tensors per step (1..{MAX_SEGMENTS}: sources x (1 + BEV levels))")
        self.keys, self.integer = [], []
        for s, lvl in self.segments:
            src, tail = self.sources[s], "" if lvl is None else f"_bev_{lvl}"
            self.keys += [f"training/{src}/{n}_iou{tail}" for n in self.class_names]
            self.keys += [f"training/{src}/{n}_count{tail}" for n in self.class_names]
            self.keys.append(f"training/{src}/source_iou{s}" if lvl is None else f"training/{src}/source_iou_bev{s}_{lvl}")
        for name in ("loss",) + self.losses:
            self.keys.append(self.loss_key(name))
        self.keys.append("training/lr")
        if len(set(self.keys)) != len(self.keys):
            raise ValueError(f"metric keys collide: sources {self.sources} must have different names")

    @classmethod
    def for_step(cls, step, sources, levels=(), **kw):
        """the layout of a step class or object of lidog_amd.trainer (its `metric_losses`, `metric_bev`,
        `metric_count_ignored`); `sources`: one name per source; `levels`: the model's BEV levels (used by LiDOGStep)"""
        sources = tuple(sources)
        names = step.metric_losses
        if len(sources) == 2:
            names = tuple(f"{n}{s}" for n in names for s in (0, 1))
        return cls(sources, names, levels if step.metric_bev else (), step.metric_count_ignored, **kw)

    def loss_key(self, name):
        if name == "loss":
            return f"training/{self.sources[0]}/total_loss"
        s, base = (int(name[-1]), name[:-1]) if name[-1].isdigit() else (0, name)
        return f"training/{self.sources[s]}/{base}{s}"

    def pack(self, counts, scalars):
        """counts [k, segments, C + 1, C], scalars [k, 1 + losses + 1] (total, the losses, lr) -> [k, 2 K] float64 on
        their device: value * flag of every key, then the flags (1 = the key is present on this rank; a class key is
        present when the class occurs in the labels).  Summed over the ranks it gives rank_mean its two sums."""
        iou, present, occ = iou_from_counts(counts, self.count_ignored)
        k, c, K = counts.shape[0], self.num_classes, len(self.keys)
        seg = len(self.segments) * (2 * c + 1)
        out = torch.ones((k, 2 * K), dtype=torch.float64, device=counts.device)     # the flags of means, losses and lr
        vals, flags = out[:, :seg].view(k, -1, 2 * c + 1), out[:, K:K + seg].view(k, -1, 2 * c + 1)
        # an absent class has IoU 0 (its intersection is empty) and 0 occurrences: value * flag is the value
        vals[..., :c] = iou
        vals[..., c:2 * c] = occ
        vals[..., 2 * c] = iou.sum(dim=-1) / occ.count_nonzero(dim=-1).clamp(min=1)
        flags[..., :c] = present
        flags[..., c:2 * c] = present
        out[:, seg:K] = scalars
        return out

    def rank_mean(self, packed):
        """[k, 2 K] sums over the ranks -> (values [k, K], present [k, K]): per key the mean over the ranks where it is
        present (sync_dist=True of log_losses); with one rank the values themselves"""
        K = len(self.keys)
        packed = torch.as_tensor(packed)
        if packed.dim() != 2 or packed.shape[1] != 2 * K:
            raise ValueError(f"rank_mean: expected [k, {2 * K}], got {tuple(packed.shape)}")
        sums, flags = packed[:, :K], packed[:, K:]
        return sums / flags.clamp(min=1), flags > 0

    def records(self, values, present, steps, epochs):
        """one dict per step: {"step": .., key: value of every present key, "training/epoch": ..}; counts as ints on
        one rank (a mean over ranks may be fractional)"""
        out = []
        for row, pres, step, epoch in zip(values.tolist(), present.tolist(), steps, epochs):
            rec = {"step": int(step)}
            for key, v, p in zip(self.keys, row, pres):
                if p:
                    rec[key] = int(v) if "_count" in key and float(v).is_integer() else v
            rec["training/epoch"] = int(epoch)
            out.append(rec)
        return out


class MetricsWriter:
    """appends one JSON object per record to `path` (<save_dir>/metrics.jsonl; rank 0 only makes one).  The file appears
    with the first record."""

    def __init__(self, path):
        self.path = path

    def write(self, record):
        d = os.path.dirname(self.path)
        if d:
            os.makedirs(d, exist_ok=True)
        with open(self.path, "a") as f:
            f.write(json.dumps(record) + "\n")

    @staticmethod
    def read(path):
        with open(path) as f:
            return [json.loads(line) for line in f if line.strip()]


class StepMetrics:
    """A device ring of `log_every_n_steps` slots; a slot holds the counts of every segment of one logged step, its
    detached loss scalars and the lr.
      record(step, pairs, losses, lr)   one lidog_train_confusion launch into the next slot and device-side copies of
                                        the scalars; nothing is read from the device (a full ring is flushed first)
      flush()    the filled slots -> per-step values on the device (MetricLayout.pack), ONE dist.all_reduce of the
                 packed vector in a data-parallel run, a non-blocking copy to a pinned buffer behind an event; then the
                 PREVIOUS flush's buffer is read.  Two buffers: a flush waits for the flush before it, whose copy was
                 queued a ring earlier, never for the step that follows it
      finish()   flush, read everything outstanding (the end of an epoch and of the run), return the records since
                 the last finish()
    Everything the ring launches runs on a stream of its own that waits for the caller's stream at record(): the
    launches of a logged step (the counts, and at a flush some thirty small operators) sit beside the step's backward
    pass, not between its forward and backward pass on the step's stream (measured there: +0.45 ms per step with every
    step logged).  The host's share of a logged step (half a millisecond when it also flushes) belongs
    where the host is ahead of the device: a step takes a mark() behind its forward pass and calls record(ready=mark)
    once its backward pass and update are queued.
    Records go to `writer` (a MetricsWriter, or None) as they are read.  The driver sets `next_step` and `epoch` before a
    step it wants recorded; left alone, next_step counts the records."""

    def __init__(self, layout, log_every_n_steps=50, ignore_label=-1, device="cuda", writer=None):
        self.layout, self.slots = layout, int(log_every_n_steps)
        if self.slots < 1:
            raise ValueError("log_every_n_steps must be at least 1")
        self.ignore_label, self.device, self.writer = int(ignore_label), torch.device(device), writer
        c, k = layout.num_classes, len(layout.keys)
        self.counts = torch.zeros((self.slots, len(layout.segments), c + 1, c), dtype=torch.int64, device=self.device)
        self.scalars = torch.zeros((self.slots, len(layout.losses) + 2), dtype=torch.float64, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.stream = torch.cuda.Stream(self.device)
        self._host = [torch.empty((self.slots, 2 * k), dtype=torch.float64).pin_memory() for _ in range(2)]
        self._host_err = [torch.zeros(1, dtype=torch.int32).pin_memory() for _ in range(2)]
        self._which, self._pending = 0, None
        self.filled, self._steps, self._epochs = 0, [], []
        self.next_step, self.epoch = 1, 0
        self._records = []
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1

    def mark(self):
        """an event on the caller's stream: what is queued so far (a step's forward pass and losses) is what a later
        record(..., ready=event) reads"""
        event = torch.cuda.Event()
        event.record()
        return event

    @torch.no_grad()
    def record(self, step, pairs, losses, lr, ready=None):
        """`pairs`: one (logits, labels) per segment in the layout's order; `losses`: {"loss": total, name: loss};
        `ready`: a mark() behind which they are complete (None: everything queued on the caller's stream so far)"""
        if self.filled == self.slots:
            self.flush()
        pairs = list(pairs)
        if len(pairs) != len(self.layout.segments):
            raise ValueError(f"StepMetrics.record: {len(pairs)} pairs for {len(self.layout.segments)} segments")
        i = self.filled
        if ready is None:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
        else:
            self.stream.wait_event(ready)
        with torch.cuda.stream(self.stream):
            train_confusion(pairs, self.layout.num_classes, self.ignore_label, out=self.counts[i], err=self.err)
            row = self.scalars[i]
            for j, name in enumerate(("loss",) + self.layout.losses):
                v = losses[name]
                if torch.is_tensor(v):
                    row[j].copy_(v.detach().reshape(()), non_blocking=True)
                    v.record_stream(self.stream)
                else:
                    row[j].fill_(float(v))
            row[-1].fill_(float(lr))
        for logits, labels in pairs:            # their memory is not handed out again before this stream has read it
            logits.record_stream(self.stream)
            labels.record_stream(self.stream)
        self._steps.append(int(step))
        self._epochs.append(int(self.epoch))
        self.filled += 1
        self.next_step = int(step) + 1

    @torch.no_grad()
    def flush(self):
        k = self.filled
        if k:
            b = self._which
            with torch.cuda.stream(self.stream):
                packed = self.layout.pack(self.counts[:k], self.scalars[:k])
                if self.world > 1:
                    dist.all_reduce(packed)              # the one collective: sums of values and of presence flags
                self._host[b][:k].copy_(packed, non_blocking=True)
                self._host_err[b].copy_(self.err, non_blocking=True)
                event = torch.cuda.Event()
                event.record()
                self.counts[:k].zero_()
            previous, self._pending = self._pending, (b, k, self._steps, self._epochs, event)
            self._which, self.filled, self._steps, self._epochs = 1 - b, 0, [], []
            self._harvest(previous)

    def _harvest(self, pending):
        if pending is None:
            return
        b, k, steps, epochs, event = pending
        event.synchronize()
        check_label_error(int(self._host_err[b][0]), "StepMetrics")
        values, present = self.layout.rank_mean(self._host[b][:k].clone())
        new = self.layout.records(values, present, steps, epochs)
        if self.writer is not None:
            for rec in new:
                self.writer.write(rec)
        self._records += new

    def finish(self):
        self.flush()
        pending, self._pending = self._pending, None
        self._harvest(pending)
        out, self._records = self._records, []
        return out
