"""Checkpoint evaluation on target domains: the reference's sixth entry script, eval_target.py.

    python -m lidog_amd.eval_target --checkpoint RUN/checkpoints/epoch=0-step=4.ckpt --targets kitti120k nusc35k
    python -m lidog_amd.eval_target --checkpoint ... --model MinkUNet34 --targets nusc35k --save-predictions
    python -m lidog_amd.eval_target --checkpoint ... --precision bf16
    python -m lidog_amd.eval_target --checkpoint ... --target-files SemanticKITTI=/data/SemanticKITTI --label-maps semantickitti2common.yaml
    python -m lidog_amd.eval_target --checkpoint ... --target-files ... --label-maps ... --point-level
    python -m lidog_amd.eval_target --checkpoint ... --target-files ... --label-maps ... --save-labels --inverse-label-map common2semantickitti.yaml
    python -m lidog_amd.eval_target --checkpoint ... --calibration --temperature fit --calibrate-on kitti120k

What the reference does through pytorch-lightning's trainer.test, as plain arguments:
  get_model / get_target_domains / loaders with batch_size * 2, shuffle=False        eval_target.py:46-89,119-167
  the checkpoint is required; save_dir = two directories above it                    eval_target.py:169-181
  test_step: one IoU row per loader BATCH, optional point clouds per scan            trainer_lighting.py:186-253,
                                                                                     trainer_lighting_bev.py:265-323
  test_epoch_end: `<save_dir>/results/<sources>-TO-<targets>.csv`                    trainer_lighting.py:255-313

The metric runs on the device up to integer confusion counts (lidog_amd.evaluate.TargetEvaluator); the counts cross to
the host once per target.  Target scans are synthetic (lidog_amd.synth), drawn as train.py draws validation scans: scan
i of target t has seed 10**6 + t * synth.SOURCE1_SEED + i.  `main(argv)` returns the per-target results.

Point level (--point-level / --save-labels, file targets only; the voxel-level outputs stay what they are): every record
of every scan file gets the class of its voxel (lidog_amd.evaluate.point_labels), records beyond the radius a fill id;
`<sources>-TO-<targets>-points.csv` holds the IoU over the labelled points, and --save-labels writes one uint32 id per
record in file order, for SemanticKITTI as `predictions/<target>/sequences/SS/predictions/NNNNNN.label`.
--point-interp trilinear: a point takes the class of the logits interpolated at its own position between the voxels
(lidog_amd.evaluate.point_logits over csrc/field.hip) instead of its voxel's; the default, nearest, changes nothing.
--tta NAME [NAME ...]: test-time augmentation (lidog_amd.tta): every batch also runs over the named views and a point
takes the arg-max of the scores accumulated over its views (--tta-mode prob / logit / vote, csrc/tta.hip); the point
table goes to `<sources>-TO-<targets>-points-tta.csv`, the voxel-level outputs stay those of the unchanged scan.
--weights averaged: evaluate the trajectory average that a run under train --weight-average stored in the checkpoint
(`averaged_state_dict`) instead of the weights of its last step; every results file then carries `-avg` before `.csv`
and predictions and labels go under `predictions-avg/`.  The default, live, writes what it always wrote.
--adapt bn / adabn / tent: test-time adaptation on the unlabelled target (lidog_amd.adapt; --adapt-lr, --adapt-optimizer,
--adapt-steps and --adapt-margin belong to tent).  The model returns to the checkpoint before every target; every results
file carries `-adapt-<mode>` before `.csv` (after `-avg`, `-points`), predictions and labels go under
`predictions<-avg>-adapt-<mode>/`.  fp32 only, one rank, not together with --tta.  The default, none, builds no adapter.
--calibration: how far the voxel softmax can be trusted (lidog_amd.calibration over csrc/calib.hip): ECE, MCE, NLL, Brier
score, accuracy and mean confidence over --calib-bins equal-width confidence bins into
`<sources>-TO-<targets>-calibration<suffix>.csv`, the per-bin table into `<sources>-TO-<targets>-reliability<suffix>.csv`
(the suffixes of --weights averaged and --adapt, as above).  --temperature VALUE scores T = 1 and T = VALUE; --temperature
fit first fits T (temperature scaling) with the checkpoint under evaluation on a labelled calibration set, the validation
scans of --calibrate-on CONFIG (synthetic, --calibrate-scans of them) or of --calibrate-files NAME=PATH with
--calibrate-label-maps, before any target runs; under --adapt the adapter runs over that set and is reset afterwards.  A
temperature moves no arg-max: every other output stays byte for byte what it is.  Voxel level only.
"""
import argparse
import json
import os
import time

import torch

from . import synth
from .checkpoint import load_lightning_checkpoint
from .evaluate import (CLASS_NAMES, PointLabelWriter, PointPath, Predictor, TargetEvaluator, dataset_batches,
                       inverse_lut, load_inverse_label_map, palette, write_ply, write_results_csv)
from . import adapt, scans, tta
from .train import SynthScans, bev_image_size, build_model, source_names

MODELS = ("MinkUNet34BEV", "MinkUNet34", "MinkUNet34IBN", "MinkUNet34Robust")
NO_CHECKPOINT = "You must provide a checkpoint for evaluation!"          # eval_target.py:174


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--checkpoint", default=None, help="checkpoint to evaluate (required); results and predictions go "
                                                       "to the directory two levels above it")
    ap.add_argument("--model", default="MinkUNet34BEV", choices=MODELS)
    ap.add_argument("--bound", type=float, default=50.0)
    ap.add_argument("--sources", nargs="+", default=["kitti120k"], metavar="NAME",
                    help="names of the training sources: the CSV's source column and file name")
    ap.add_argument("--targets", nargs="+", default=["nusc35k"], choices=sorted(synth.CONFIGS), metavar="CONFIG",
                    help="one or two target configurations")
    ap.add_argument("--scans", type=int, default=16, help="scans per target")
    ap.add_argument("--batch", type=int, default=8, help="loader batch: twice train's, as eval_target.py doubles it")
    ap.add_argument("--rows", default="batch", choices=["batch", "scan"],
                    help="one IoU row per loader batch (the reference) or per scan")
    ap.add_argument("--save-predictions", action="store_true")
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--precision", default="fp32", choices=["fp32", "bf16"],
                    help="bf16: convolutions with channel counts that are multiples of 32 multiply bf16 operands "
                         "(fp32 accumulation, fp32 activations); the weights are packed once per target")
    scans.add_file_arguments(ap, "--target-files", "evaluate on the validation")
    ap.add_argument("--point-level", action="store_true",
                    help="with --target-files: also score one label per point of every scan file (records beyond the "
                         "radius are left out) into <sources>-TO-<targets>-points.csv")
    ap.add_argument("--save-labels", action="store_true",
                    help="with --target-files: write one uint32 id per record of every scan file, in file order "
                         "(SemanticKITTI: predictions/<target>/sequences/SS/predictions/NNNNNN.label)")
    ap.add_argument("--point-interp", default="nearest", choices=["nearest", "trilinear"],
                    help="with --point-level / --save-labels: a point takes its voxel's class (nearest) or the class of the "
                         "logits interpolated trilinearly at its own position (missing neighbours add nothing)")
    ap.add_argument("--tta", nargs="+", default=None, metavar="NAME",
                    help="with --point-level / --save-labels: test-time augmentation.  Every batch also runs over these "
                         "views and a point takes the class its views agree on.  A view is a '+'-joined list of "
                         "rotz<deg>, flipx, flipy, scale<f>; presets rot4 (rotz90 rotz180 rotz270) and flip4 (flipx "
                         "flipy flipx+flipy); the unchanged scan is always view 0.  The point table then goes to "
                         "<sources>-TO-<targets>-points-tta.csv")
    ap.add_argument("--tta-mode", default=None, choices=list(tta.MODES),
                    help="with --tta: what the views add up per point: softmax probabilities (prob, the default), logits "
                         "or one vote per view for its arg-max")
    ap.add_argument("--inverse-label-map", nargs="+", default=None, metavar="FILE",
                    help="one per target: a .yaml / .json file with a learning_map_inv (common class -> id to write; "
                         "entry -1: the id of records beyond the radius, default 0).  Default: the class itself")
    ap.add_argument("--weights", default="live", choices=["live", "averaged"],
                    help="which weights of the checkpoint to evaluate: those of its last step (live, the default) or the "
                         "trajectory average a run under train --weight-average stored next to them (averaged: every "
                         "results file gets -avg before .csv, predictions and labels go under predictions-avg/)")
    ap.add_argument("--adapt", default="none", choices=["none"] + list(adapt.MODES),
                    help="test-time adaptation on the unlabelled target (lidog_amd.adapt): bn normalises every batch with "
                         "its own statistics, adabn re-estimates the BatchNorm running statistics over the target's "
                         "batches before the scored pass, tent also takes gradient steps on the norm layers' affine "
                         "parameters that lower the entropy of every batch's predictions.  The model returns to the "
                         "checkpoint before every target; every results file gets -adapt-<mode> before .csv")
    ap.add_argument("--adapt-lr", type=float, default=None, help="with --adapt tent: the learning rate (default 1e-3)")
    ap.add_argument("--adapt-optimizer", default=None, choices=["Adam", "SGD"], help="with --adapt tent (default Adam)")
    ap.add_argument("--adapt-steps", type=int, default=None,
                    help="with --adapt tent: gradient steps per batch (default 1)")
    ap.add_argument("--adapt-margin", type=float, default=None, metavar="F",
                    help="with --adapt tent: only voxels whose entropy lies below F ln C enter the loss (EATA / SAR use "
                         "0.4; default: every voxel)")
    ap.add_argument("--calibration", action="store_true",
                    help="also report the calibration of the voxel softmax (ECE, MCE, NLL, Brier, accuracy, mean "
                         "confidence) into <sources>-TO-<targets>-calibration.csv and the per-bin table into "
                         "<sources>-TO-<targets>-reliability.csv")
    ap.add_argument("--calib-bins", type=int, default=None, metavar="B",
                    help="with --calibration: equal-width confidence bins, 1..64 (default 15)")
    ap.add_argument("--temperature", default=None, metavar="VALUE|fit",
                    help="with --calibration: also score softmax(logits / T); a value in 0.01..100, or `fit`: temperature "
                         "scaling fitted on the calibration set (--calibrate-on or --calibrate-files) before any target runs")
    ap.add_argument("--calibrate-on", default=None, choices=sorted(synth.CONFIGS), metavar="CONFIG",
                    help="with --temperature fit: fit on the synthetic validation scans of this configuration")
    ap.add_argument("--calibrate-scans", type=int, default=None, metavar="N",
                    help="with --temperature fit: scans of the calibration set (default 16; the first N files of "
                         "--calibrate-files)")
    ap.add_argument("--calibrate-files", default=None, metavar="NAME=PATH",
                    help="with --temperature fit: fit on the validation scans of this dataset (names as --target-files)")
    ap.add_argument("--calibrate-label-maps", default=None, metavar="FILE",
                    help="the label map of --calibrate-files")
    a = ap.parse_args(argv)
    if a.checkpoint is None:
        ap.error(NO_CHECKPOINT)
    check_calibration_arguments(ap, a)
    if a.adapt != "tent" and any(v is not None for v in (a.adapt_lr, a.adapt_optimizer, a.adapt_steps, a.adapt_margin)):
        ap.error("--adapt-lr, --adapt-optimizer, --adapt-steps and --adapt-margin go with --adapt tent")
    if a.adapt != "none":
        if a.precision == "bf16":
            ap.error("--adapt goes with --precision fp32 (test-time adaptation is fp32 only)")
        if a.tta is not None:
            ap.error("--adapt and --tta exclude each other (the views of a scan would not be adapted)")
    if a.adapt == "tent":
        a.adapt_lr = 1e-3 if a.adapt_lr is None else a.adapt_lr
        a.adapt_optimizer = a.adapt_optimizer or "Adam"
        a.adapt_steps = 1 if a.adapt_steps is None else a.adapt_steps
        if a.adapt_steps < 1 or not a.adapt_lr >= 0 or (a.adapt_margin is not None and not a.adapt_margin > 0):
            ap.error("--adapt-steps must be positive, --adapt-lr non-negative and --adapt-margin positive")
    if a.target_files is not None:
        a.target_files = scans.check_file_arguments(ap, a.target_files, a, "--target-files")
        a.targets = [n for n, _ in a.target_files]               # the CSV's target names
    elif a.label_maps is not None or (a.synth4d_splits is not None and a.calibrate_files is None) or \
            a.limit_files is not None:
        ap.error("--label-maps, --synth4d-splits and --limit-files go with --target-files")
    if (a.point_level or a.save_labels or a.inverse_label_map is not None) and a.target_files is None:
        ap.error("--point-level, --save-labels and --inverse-label-map go with --target-files (a synthetic target has no "
                 "file whose order the labels could follow)")
    if a.point_interp != "nearest" and not (a.point_level or a.save_labels):
        ap.error("--point-interp goes with --point-level or --save-labels")
    if a.tta_mode is not None and a.tta is None:
        ap.error("--tta-mode goes with --tta")
    if a.tta is not None:
        if a.target_files is None or not (a.point_level or a.save_labels):
            ap.error("--tta goes with --target-files and --point-level or --save-labels (the views are voted per point)")
        if a.point_interp != "nearest":
            ap.error("--tta goes with --point-interp nearest (per-view interpolation is not built)")
        try:
            tta.parse_views(a.tta)
        except ValueError as e:
            ap.error(f"--tta: {e}")
    a.tta_mode = a.tta_mode or "prob"
    if a.inverse_label_map is not None:
        if len(a.inverse_label_map) != len(a.target_files):
            ap.error("--inverse-label-map needs one file per --target-files entry")
    if len(a.targets) > 2:
        raise NotImplementedError(f"{len(a.targets)} targets (the reference takes one or two)")
    if a.scans < 1 or a.batch < 1:
        ap.error("--scans and --batch must be positive")
    return a


T_MIN, T_MAX = 0.01, 100.0


def check_calibration_arguments(ap, a):
    """the refusals of --calibration and what goes with it; a.temperature becomes None, "fit" or a float, the defaults
    of --calib-bins and --calibrate-scans are filled in, a.calibrate_files becomes (name, path)"""
    sets = (a.calibrate_on is not None) + (a.calibrate_files is not None)
    if not a.calibration:
        if a.calib_bins is not None or a.temperature is not None or sets or a.calibrate_scans is not None or \
                a.calibrate_label_maps is not None:
            ap.error("--calib-bins, --temperature, --calibrate-on, --calibrate-scans, --calibrate-files and "
                     "--calibrate-label-maps go with --calibration")
        return
    a.calib_bins = 15 if a.calib_bins is None else a.calib_bins
    if not 1 <= a.calib_bins <= 64:
        ap.error("--calib-bins must lie in 1..64")
    if a.temperature is not None and a.temperature != "fit":
        try:
            a.temperature = float(a.temperature)
        except ValueError:
            ap.error(f"--temperature: {a.temperature!r} is neither a number nor `fit`")
        if not a.temperature > 0:
            ap.error("--temperature must be positive")
        if not T_MIN <= a.temperature <= T_MAX:
            ap.error(f"--temperature must lie in {T_MIN}..{T_MAX:g}")
    if a.temperature == "fit":
        if sets != 1:
            ap.error("--temperature fit needs exactly one calibration set: --calibrate-on CONFIG or --calibrate-files "
                     "NAME=PATH")
    elif sets or a.calibrate_scans is not None or a.calibrate_label_maps is not None:
        ap.error("--calibrate-on, --calibrate-scans, --calibrate-files and --calibrate-label-maps go with --temperature fit")
    if a.temperature == "fit":
        a.calibrate_scans = 16 if a.calibrate_scans is None else a.calibrate_scans
        if a.calibrate_scans < 1:
            ap.error("--calibrate-scans must be positive")
        if (a.calibrate_files is None) != (a.calibrate_label_maps is None):
            ap.error("--calibrate-files and --calibrate-label-maps go together")
        if a.calibrate_files is not None:
            try:
                files = scans.parse_files([a.calibrate_files])
            except ValueError as e:
                ap.error(f"--calibrate-files: {e}")
            if "Synth4D" in files[0][0] and a.synth4d_splits is None:
                ap.error("--calibrate-files: a Synth4D entry needs --synth4d-splits")
            a.calibrate_files = files[0]


def calibration_set(a, bev):
    """the labelled scans --temperature fit fits on: validation scans, as train draws them for its first source"""
    if a.calibrate_files is not None:
        name, path = a.calibrate_files
        return scans.FileScans(scans.listing(name, path, "validation", version=a.version,
                                             synth4d_splits=a.synth4d_splits, limit=a.calibrate_scans),
                               scans.luts_from_files([a.calibrate_label_maps])[0])
    return SynthScans(a.calibrate_scans, a.calibrate_on, first=10 ** 6, bev_size=bev)


def fit_on_calibration_set(a, model, adapter, bev, device):
    """(Temperature, its calibration metrics at T = 1 and at the fitted T) of the checkpoint on calibration_set(a): the
    logits are those a target would be scored on (--precision, --adapt; the adapter is reset before and after)"""
    from . import calibration
    data = calibration_set(a, bev)
    if adapter is not None:
        adapter.reset()
        if a.adapt == "adabn":
            adapter.estimate(dataset_batches(data, a.batch, device))
    run = adapter if adapter is not None else Predictor(model, a.precision)
    logits, labels = calibration.collect_logits(run, dataset_batches(data, a.batch, device))
    if adapter is not None:
        adapter.reset()
    fit = calibration.fit_temperature(logits, labels, beta_min=1.0 / T_MAX, beta_max=1.0 / T_MIN)
    own = {}
    for name, beta in (("raw", None), ("scaled", fit.beta)):
        own[name] = calibration.CalibrationTable(a.calib_bins, logits.device).add(logits, labels, beta=beta).result()
    if fit.summary()["rows"] == 0:
        raise SystemExit("eval_target --temperature fit: the calibration set has no labelled voxel")
    return fit, own


def save_dir_of(checkpoint):
    """eval_target.py:176-177: the checkpoint's directory is `<save_dir>/checkpoints`"""
    return os.path.split(os.path.split(checkpoint)[0])[0]


class PredictionWriter:
    """the point clouds of test_step: `<folder>/<target>/preds/<idx>.ply` coloured by prediction, and, except for the
    BEV model (trainer_lighting_bev.py:293-320 writes only preds), `<folder>/<target>/labels/<idx>.ply` coloured by
    label.  The points are the integer voxel coordinates, as the reference writes them."""

    def __init__(self, folder, target, with_labels, num_classes=7):
        self.dirs = {"preds": os.path.join(folder, target, "preds")}
        if with_labels:
            self.dirs["labels"] = os.path.join(folder, target, "labels")
        for d in self.dirs.values():
            os.makedirs(d, exist_ok=True)
        self.colors = palette(num_classes)

    def __call__(self, idx, rec):
        write_ply(os.path.join(self.dirs["preds"], f"{idx}.ply"), rec[:, :3], self.colors[rec[:, 3] + 1])
        if "labels" in self.dirs:
            write_ply(os.path.join(self.dirs["labels"], f"{idx}.ply"), rec[:, :3], self.colors[rec[:, 4] + 1])


def main(argv=None):
    a = parse_args(argv)
    torch.manual_seed(a.seed)
    device = "cuda"
    model = build_model(a.model, a.bound, device=device)
    try:
        epoch, _ = load_lightning_checkpoint(model, a.checkpoint, which=a.weights)
    except KeyError as e:
        if a.weights != "averaged":
            raise
        raise SystemExit(f"eval_target --weights averaged: {e.args[0]}")
    avg = "-avg" if a.weights == "averaged" else ""      # the two kinds never share a table or a folder
    adapter = None
    if a.adapt != "none":                                # an adapted run never shares a table or a folder either
        avg += f"-adapt-{a.adapt}"
    model.eval()
    if a.adapt == "tent":
        import math
        adapter = adapt.TestTimeAdapter(model, "tent", lr=a.adapt_lr, optimizer=a.adapt_optimizer, steps=a.adapt_steps,
                                        margin=None if a.adapt_margin is None else
                                        a.adapt_margin * math.log(len(CLASS_NAMES)))
    elif a.adapt != "none":
        adapter = adapt.TestTimeAdapter(model, a.adapt)
    save_dir = save_dir_of(a.checkpoint)
    sources = "".join(source_names(a.sources))                       # test_epoch_end concatenates the names
    targets = source_names(a.targets)
    file_targets = "".join(targets)
    bev = bev_image_size(a.bound)
    ev = TargetEvaluator(model, num_classes=len(CLASS_NAMES), precision=a.precision, adapter=adapter)
    results = []
    calib = fit = None                                   # [(name, beta)] of TargetEvaluator.run, and their temperatures
    if a.calibration:
        from . import calibration
        calib, temps = [("raw", None)], [1.0]
        if a.temperature == "fit":
            fit, fit_own = fit_on_calibration_set(a, model, adapter, bev, device)
            calib.append(("scaled", fit.beta))
            temps.append(fit.temperature())
        elif a.temperature is not None:
            calib.append(("scaled", torch.tensor([1.0 / a.temperature], dtype=torch.float64, device=device)))
            temps.append(a.temperature)
    luts = None
    if a.target_files is not None:
        luts = scans.luts_from_files(a.label_maps)
    for t, (name, config) in enumerate(zip(targets, a.targets)):
        if luts is not None:      # the validation listing of the target, every kept point, voxelised
            data = scans.FileScans(scans.listing(config, a.target_files[t][1], "validation", version=a.version,
                                                 synth4d_splits=a.synth4d_splits, limit=a.limit_files), luts[t])
        else:
            data = SynthScans(a.scans, config, first=10 ** 6 + t * synth.SOURCE1_SEED, bev_size=bev)
        points = None
        if a.point_level or a.save_labels:
            lut, fill = inverse_lut(load_inverse_label_map(a.inverse_label_map[t]) if a.inverse_label_map else None,
                                    len(CLASS_NAMES), 0xFFFF if config == "SemanticKITTI" else 2 ** 31 - 1)
            label_writer = None
            if a.save_labels:
                label_writer = PointLabelWriter(os.path.join(save_dir, "predictions" + avg), name, config,
                                                data.listings[0].files)
            points = PointPath.of(data, device, out_lut=torch.from_numpy(lut).to(device), fill=fill,
                                  with_labels=a.point_level, on_point_labels=label_writer, interp=a.point_interp, tta=a.tta,
                                  tta_mode=a.tta_mode)
        writer = None
        if a.save_predictions:
            writer = PredictionWriter(os.path.join(save_dir, "predictions" + avg), name, a.model != "MinkUNet34BEV",
                                      len(CLASS_NAMES))
        if adapter is not None:
            adapter.reset()                              # no target sees what another one left in the model
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if a.adapt == "adabn":                           # part of the target's time: the scans go through twice
            adapter.estimate(dataset_batches(data, a.batch, device))
        res = ev.run(dataset_batches(data, a.batch, device), len(data), rows=a.rows, on_predictions=writer,
                     points=points, calibration=calib, calib_bins=a.calib_bins or 15)
        dt = time.perf_counter() - t0                                # run() ends with the host copy of the counts
        path = write_results_csv(save_dir, sources, name, res["rows"], CLASS_NAMES, first_target=t == 0,
                                 file_targets=file_targets + avg)
        out = {"target": name, "checkpoint_epoch": epoch, "per_class_iou": [float(x) for x in res["per_class"]],
               "mean_iou": res["mean"], "rows": int(res["rows"].shape[0]), "rows_per": a.rows,
               "scans": int(res["scans"]), "scans_per_s": res["scans"] / dt, "csv": path}
        extra = {}
        if a.point_level:
            out["points_csv"] = write_results_csv(save_dir, sources, name, res["point_rows"], CLASS_NAMES,
                                                  first_target=t == 0, file_targets=file_targets +
                                                  ("-points-tta" if a.tta is not None else "-points") + avg)
            out["point_per_class_iou"] = [float(x) for x in res["point_per_class"]]
            out["point_mean_iou"] = res["point_mean"]
            extra = {"point_iou_rows": res["point_rows"], "point_counts": res["point_counts"]}
        if a.save_labels:
            out["label_files"] = len(points.on_point_labels.written)
            extra["label_paths"] = list(points.on_point_labels.written)
        if a.tta is not None:
            out.update(tta_views=res["tta_views"], tta_mode=res["tta_mode"])
        if adapter is not None:
            out.update(adapt=a.adapt, adapt_lr=a.adapt_lr, adapt_steps=a.adapt_steps)
        if calib is not None:
            entries = [(temp, res["calibration"][n]) for temp, (n, _) in zip(temps, calib)]
            out["calibration_csv"] = calibration.write_calibration_csv(
                save_dir, sources, name, entries, first_target=t == 0, file_targets=file_targets + "-calibration" + avg)
            out["reliability_csv"] = calibration.write_reliability_csv(
                save_dir, sources, name, entries, first_target=t == 0, file_targets=file_targets + "-reliability" + avg)
            out["calibration"] = {n: {k: m[k] for k in calibration.METRICS + ("rows",)}
                                  for n, m in res["calibration"].items()}
            extra["calibration_tables"] = res["calibration"]
            if len(temps) > 1:
                out["temperature"] = temps[1]
            if fit is not None:
                out["temperature_fit"] = {"on": a.calibrate_on or a.calibrate_files[0], "scans": a.calibrate_scans,
                                          "nll_raw": fit_own["raw"]["nll"], "nll_scaled": fit_own["scaled"]["nll"],
                                          "rows": fit_own["raw"]["rows"]}
        print(json.dumps(out), flush=True)
        results.append(dict(out, iou_rows=res["rows"], counts=res["counts"], **extra))
    return results


if __name__ == "__main__":
    main()
