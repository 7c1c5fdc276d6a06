"""Calibration of the voxel softmax: reliability table, ECE / MCE / NLL / Brier, and temperature scaling.

    table = CalibrationTable(n_bins=15)
    for logits, labels in batches:
        table.add(logits, labels)                       # one launch (csrc/calib.hip), nothing read back
    m = table.result()                                  # the one read-back: ece, mce, nll, brier, accuracy, ...

    fit = fit_temperature(cal_logits, cal_labels)       # 24 launches queued back to back (Guo et al., ICML 2017)
    scaled = CalibrationTable()
    scaled.add(logits, labels, beta=fit.beta)           # the fitted word is used where it lies, on the device
    fit.temperature()                                   # a host float: reads once

include/lidog_amd.h states the arithmetic.  The kernel accumulates integers (counts, and confidences and Brier scores in
units of 2^-32) so that a table does not depend on how a dataset is cut into batches; `metrics_from_table` turns the
accumulators into the metrics on the host, in float64, and needs no GPU:
    ECE = sum_b (n_b / N) |acc_b - conf_b|,  MCE = max over non-empty bins of |acc_b - conf_b|
over B equal-width confidence bins, confidence = the largest softmax probability.  Voxel level only: points of one voxel
can carry different labels, and test-time-augmentation scores are not logits."""
import numpy as np
import torch

MAX_CLASSES = 32
MAX_BINS = 64
Q = 4294967296.0                    # 2^32: the unit of conf_q and brier_q
ERR_NONFINITE = 2
STATE = ("beta", "lo", "hi", "nll", "g", "h", "iterations", "rows")
METRICS = ("ece", "mce", "nll", "brier", "accuracy", "confidence")


def metrics_from_table(table, totals, nll_sum):
    """The metrics of lidog_calib_stats' accumulators, in float64 on the host: table [B, 3] int64 (count, correct,
    conf_q), totals [2] int64 (rows, brier_q), nll_sum a float.  Returns a dict: ece, mce, nll, brier, accuracy,
    confidence (the mean one), rows, and reliability [B, 4] float64 = (bin lower edge, count, accuracy, mean confidence),
    the last two 0 in an empty bin.  rows == 0 gives zeros, never a NaN."""
    table = np.asarray(table, dtype=np.int64)
    totals = np.asarray(totals, dtype=np.int64).reshape(-1)
    if table.ndim != 2 or table.shape[1] != 3 or table.shape[0] < 1 or totals.shape != (2,):
        raise ValueError(f"metrics_from_table: table [B, 3] and totals [2], got {table.shape} and {totals.shape}")
    b = table.shape[0]
    count = table[:, 0].astype(np.float64)
    rows = int(totals[0])
    if int(table[:, 0].sum()) != rows:
        raise ValueError(f"metrics_from_table: the bins hold {int(table[:, 0].sum())} rows, totals says {rows}")
    full = table[:, 0] > 0
    safe = np.where(full, count, 1.0)
    acc = np.where(full, table[:, 1] / safe, 0.0)
    conf = np.where(full, (table[:, 2] / Q) / safe, 0.0)
    gap = np.abs(acc - conf)
    rel = np.stack([np.arange(b, dtype=np.float64) / b, count, acc, conf], axis=1)
    if rows == 0:
        return dict(ece=0.0, mce=0.0, nll=0.0, brier=0.0, accuracy=0.0, confidence=0.0, rows=0, reliability=rel)
    return dict(ece=float((count / rows * gap).sum()), mce=float(gap[full].max()), nll=float(nll_sum) / rows,
                brier=float(totals[1]) / Q / rows, accuracy=float(table[:, 1].sum()) / rows,
                confidence=float(table[:, 2].sum()) / Q / rows, rows=rows, reliability=rel)


def _check_rows(who, logits, labels):
    from ._lib import require_gpu
    require_gpu(logits, "logits")
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"{who}: logits must be float32 [N, C], got {logits.dtype} {tuple(logits.shape)}")
    n, c = logits.shape
    if not 2 <= c <= MAX_CLASSES:
        raise ValueError(f"{who}: {c} classes (2..{MAX_CLASSES})")
    if labels.shape != (n,) or labels.dtype != torch.int64 or labels.device != logits.device:
        raise ValueError(f"{who}: labels must be int64 [{n}] on {logits.device}, got {labels.dtype} "
                         f"{tuple(labels.shape)} on {labels.device}")
    if n * c >= 2 ** 31:
        raise ValueError(f"{who}: N * C = {n * c} reaches 2^31")
    return n, c


def _check_beta(who, beta, device):
    if beta is None:
        return None
    if isinstance(beta, Temperature):
        beta = beta.beta
    if not torch.is_tensor(beta) or beta.dtype != torch.float64 or beta.numel() != 1 or beta.device != device:
        raise ValueError(f"{who}: beta is a float64 device word on {device} (fit_temperature(...).beta, or "
                         "torch.tensor([1 / T], dtype=torch.float64, device=...)), or None for 1")
    return beta


def _workspace(ws, n, device):
    """a zeroed workspace of at least lidog_calib_ws(n) doubles (every call leaves its ticket word zero)"""
    from . import _lib
    need = int(_lib.load().lidog_calib_ws(int(n)))
    if ws is None or ws.numel() < need:
        ws = torch.zeros(need, dtype=torch.float64, device=device)
    return ws


class CalibrationTable:
    """The accumulators of lidog_calib_stats and their error word, on `device`: table [n_bins, 3] int64, totals [2]
    int64, nll_sum [1] float64.  add() is one launch and reads nothing back; result() is the one read-back."""

    def __init__(self, n_bins=15, device="cuda"):
        n_bins = int(n_bins)
        if not 1 <= n_bins <= MAX_BINS:
            raise ValueError(f"CalibrationTable: n_bins={n_bins} (1..{MAX_BINS})")
        self.n_bins, self.device = n_bins, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"lidog_amd: a CalibrationTable lives on the GPU (got {self.device}); there is no CPU "
                               "path (metrics_from_table needs none)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = torch.zeros((n_bins, 3), dtype=torch.int64, device=self.device)
        self.totals = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.nll_sum = torch.zeros(1, dtype=torch.float64, device=self.device)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ws = None

    def add(self, logits, labels, beta=None, ignore_label=-1):
        """adds the labelled rows of logits [N, C] float32 / labels [N] int64; `beta`: the inverse temperature as a
        device float64 word (or a fit_temperature result), None for 1"""
        from ._lib import call, ptr
        n, c = _check_rows("CalibrationTable.add", logits, labels)
        if logits.device != self.device:
            raise ValueError(f"CalibrationTable.add: logits on {logits.device}, the table on {self.device}")
        beta = _check_beta("CalibrationTable.add", beta, self.device)
        if n == 0:
            return self
        self._ws = _workspace(self._ws, n, self.device)
        call("lidog_calib_stats", ptr(logits.contiguous()), ptr(labels.contiguous()), n, c, int(ignore_label), ptr(beta),
             self.n_bins, ptr(self.table), ptr(self.totals), ptr(self.nll_sum), ptr(self.err), ptr(self._ws))
        return self

    def host(self):
        """(table, totals, nll_sum, err) on the host: one copy"""
        buf = torch.cat([self.table.reshape(-1), self.totals, self.nll_sum.view(torch.int64),
                         self.err.to(torch.int64)]).cpu().numpy()
        k = 3 * self.n_bins
        return buf[:k].reshape(-1, 3).copy(), buf[k:k + 2].copy(), float(buf[k + 2:k + 3].view(np.float64)[0]), \
            int(buf[k + 3])

    def result(self):
        """metrics_from_table of the accumulators; raises when a labelled row held a NaN or an infinite logit (such rows
        were left out)"""
        table, totals, nll_sum, err = self.host()
        if err & ERR_NONFINITE:
            raise ValueError("CalibrationTable: a labelled row holds a NaN or infinite logit (or beta is no positive "
                             "finite number); such rows were not counted")
        return metrics_from_table(table, totals, nll_sum)


class Temperature:
    """What fit_temperature returns.  `beta`: the fitted inverse temperature, a float64 device word (a view of `state`)
    that CalibrationTable.add takes as it is; `state` [8] and `trace_rows` [iters, 3] stay on the device until asked."""

    def __init__(self, state, trace, err):
        self.state, self.trace_rows, self.err = state, trace, err
        self.beta = state[:1]

    def _check(self):
        if int(self.err.item()) & ERR_NONFINITE:
            raise ValueError("fit_temperature: a labelled row holds a NaN or infinite logit; such rows were left out")

    def temperature(self):
        """T = 1 / beta as a host float (one read)"""
        self._check()
        return 1.0 / float(self.state[0].item())

    def summary(self):
        """the state by name: beta, lo, hi, nll, g, h (those of the last evaluated beta), iterations, rows"""
        self._check()
        return dict(zip(STATE, (float(v) for v in self.state.cpu().numpy())))

    def trace(self):
        """[iters, 3] float64 on the host: (beta used, NLL there, gradient there) of every iteration"""
        return self.trace_rows.cpu().numpy()


def fit_temperature(logits, labels, iters=24, ignore_label=-1, beta_min=0.01, beta_max=100.0):
    """Temperature scaling: minimises the NLL of softmax(beta * logits) over the labelled rows by `iters` bracketed
    Newton iterations, one launch each (lidog_calib_fit_step), queued back to back with nothing read back.  A set with
    no labelled row leaves beta = 1; one on which the gradient keeps its sign ends at beta_min or beta_max."""
    from ._lib import call, ptr
    n, c = _check_rows("fit_temperature", logits, labels)
    iters = int(iters)
    if iters < 1:
        raise ValueError(f"fit_temperature: iters={iters} (at least 1)")
    if not 0 < beta_min <= beta_max < float("inf"):
        raise ValueError(f"fit_temperature: 0 < beta_min <= beta_max (got {beta_min}, {beta_max})")
    dev = logits.device
    logits, labels = logits.contiguous(), labels.contiguous()
    state = torch.empty(8, dtype=torch.float64, device=dev)
    trace = torch.zeros((iters, 3), dtype=torch.float64, device=dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _workspace(None, n, dev)
    call("lidog_calib_fit_init", ptr(state), float(beta_min), float(beta_max))
    for i in range(iters):
        call("lidog_calib_fit_step", ptr(logits), ptr(labels), n, c, int(ignore_label), float(beta_min),
             float(beta_max), ptr(state), trace[i].data_ptr(), ptr(err), ptr(ws))
    return Temperature(state, trace, err)


@torch.no_grad()
def collect_logits(run, batches):
    """(logits [N, C] float32, labels [N] int64) on the device: `run` (an evaluate.Predictor, or an
    adapt.TestTimeAdapter in its scoring role) over `batches` (batch dicts, or the (batch, scan indices) pairs of
    evaluate.dataset_batches), concatenated in order.  Refuses a set whose N * C would reach 2^31."""
    logits, labels, n = [], [], 0
    it = iter(batches)
    cur = next(it, None)
    while cur is not None:
        nxt = next(it, None)
        b = cur[0] if isinstance(cur, (tuple, list)) else cur
        nb = None if nxt is None else (nxt[0] if isinstance(nxt, (tuple, list)) else nxt)["coords_int"]
        _, out = run(b["coords_int"], b["source_features0"], nb)
        n += out.shape[0]
        if n * out.shape[1] >= 2 ** 31:
            raise ValueError(f"collect_logits: N * C = {n * out.shape[1]} reaches 2^31; fit on fewer scans")
        logits.append(out.detach())
        labels.append(b["source_sem_labels0"])
        cur = nxt
    if not logits:
        raise ValueError("collect_logits: no batches")
    return torch.cat(logits).contiguous(), torch.cat(labels).contiguous()


# ------------------------------------------------------------------ the result files of eval_target --calibration
def _comma(x, digits=4):
    return f"{x:.{digits}f}".replace(".", ",")


def write_calibration_csv(save_dir, source_names, target_name, entries, first_target=True, file_targets=None):
    """`<save_dir>/results/<sources>-TO-<targets>-calibration<suffix>.csv`, appended: one row per target and temperature,
    `entries` = [(T, metrics)], in write_results_csv's format (decimal comma), four decimals.  Returns the path."""
    import csv
    import os
    os.makedirs(os.path.join(save_dir, "results"), exist_ok=True)
    path = os.path.join(save_dir, "results",
                        f"{source_names}-TO-{target_name if file_targets is None else file_targets}.csv")
    with open(path, "a") as f:
        w = csv.writer(f)
        if first_target:
            w.writerow(["source", "target", "T", "ECE", "MCE", "NLL", "Brier", "accuracy", "confidence"])
        for t, m in entries:
            w.writerow([source_names, target_name, _comma(t)] + [_comma(m[k]) for k in METRICS])
    return path


def write_reliability_csv(save_dir, source_names, target_name, entries, first_target=True, file_targets=None):
    """`<save_dir>/results/<sources>-TO-<targets>-reliability<suffix>.csv`, appended: one row per target, temperature and
    bin: the bin's lower edge, its row count, accuracy and mean confidence.  Returns the path."""
    import csv
    import os
    os.makedirs(os.path.join(save_dir, "results"), exist_ok=True)
    path = os.path.join(save_dir, "results",
                        f"{source_names}-TO-{target_name if file_targets is None else file_targets}.csv")
    with open(path, "a") as f:
        w = csv.writer(f)
        if first_target:
            w.writerow(["source", "target", "T", "bin", "count", "accuracy", "confidence"])
        for t, m in entries:
            for edge, count, acc, conf in m["reliability"]:
                w.writerow([source_names, target_name, _comma(t), _comma(edge), str(int(count)), _comma(acc),
                            _comma(conf)])
    return path
