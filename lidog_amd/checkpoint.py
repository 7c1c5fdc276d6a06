"""Checkpoint interchange with the reference's Lightning runs.

Lightning's ModelCheckpoint (train_lidog.py:222-225) stores `state_dict` with the LightningModule attribute
prefix `model.` (utils/pipelines/trainer_lighting_2d.py:42); parameter names below that prefix are identical to
lidog_amd.MinkUNet34 / MinkUNet34BEV (checked against the reference classes in tests/golden)."""
import torch


AVERAGED_KEY, AVERAGE_STATE_KEY = "averaged_state_dict", "weight_average"


def model_state_dict(ckpt, which="live"):
    """state_dict of the bare model from a Lightning checkpoint dict (or a plain state_dict).  `which`: "live" (the
    weights of the last step) or "averaged" (the trajectory average a run under --weight-average stores next to them)"""
    if which not in ("live", "averaged"):
        raise ValueError(f"which={which!r} (one of 'live', 'averaged')")
    if which == "averaged":
        if AVERAGED_KEY not in ckpt:
            raise KeyError(f"the checkpoint has no `{AVERAGED_KEY}`: it was not written by a run with --weight-average")
        sd = ckpt[AVERAGED_KEY]
    else:
        sd = ckpt.get("state_dict", ckpt)
    if any(k.startswith("model.") for k in sd):
        sd = {k[len("model."):]: v for k, v in sd.items() if k.startswith("model.")}
    return sd


def load_lightning_checkpoint(model, path, strict=True, map_location="cpu", which="live"):
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    missing = model.load_state_dict(model_state_dict(ckpt, which), strict=strict)
    return ckpt.get("epoch"), missing


def _cpu(v):
    if torch.is_tensor(v):
        return v.detach().cpu()
    if isinstance(v, dict):
        return {k: _cpu(x) for k, x in v.items()}
    return v


def save_lightning_checkpoint(model, path, epoch=0, global_step=0, optimizer=None, scheduler=None,
                              weight_average=None, mixstyle=None):
    """writes the keys eval_target.py / --auto_resume of the reference read back (`epoch`, `global_step`,
    `state_dict` with the `model.` prefix) plus Lightning's `optimizer_states` / `lr_schedulers` lists
    (trainer.fit(ckpt_path=...), train_lidog.py:298-301).  `optimizer_states[0]` is in torch.optim's own layout
    (`state` + `param_groups`, lidog_amd.optim._FlatOptimizer.torch_state_dict), so torch.optim.Adam / SGD over the
    reference model's parameters can load it and a checkpoint written by the reference loads here; the scheduler entry
    carries `last_epoch` (the only field both sides need).
    `weight_average` (an optim.WeightAverage that has been updated) adds two top-level keys, which Lightning and the
    reference ignore: `averaged_state_dict` (the averaged model, `model.` prefix like `state_dict`) and `weight_average`
    (its mode, decay schedule and update count).  `mixstyle` (a dict: layers, p, alpha of a run trained with MixStyle)
    is recorded as it is under the top-level key `mixstyle`; the modules have no state."""
    ckpt = {"epoch": epoch, "global_step": global_step,
            "state_dict": {"model." + k: v.detach().cpu() for k, v in model.state_dict().items()}}
    if optimizer is not None:
        to_torch = getattr(optimizer, "torch_state_dict", None)
        ckpt["optimizer_states"] = [_cpu(to_torch() if to_torch is not None else optimizer.state_dict())]
    if scheduler is not None:
        ckpt["lr_schedulers"] = [scheduler.state_dict()]
    if weight_average is not None and weight_average.num_updates > 0:
        ckpt[AVERAGED_KEY] = {"model." + k: v for k, v in weight_average.averaged_state_dict().items()}
        ckpt[AVERAGE_STATE_KEY] = weight_average.state_dict()
    if mixstyle is not None:
        ckpt["mixstyle"] = dict(mixstyle)
    tmp = path + ".tmp"
    torch.save(ckpt, tmp)
    import os
    os.replace(tmp, path)     # a killed run never leaves a truncated checkpoint behind for --auto_resume


def load_training_checkpoint(model, path, optimizer=None, scheduler=None, map_location="cpu", weight_average=None):
    """model + optimiser state + scheduler position of a checkpoint written by save_lightning_checkpoint; returns the
    checkpoint dict (`epoch` = the epoch that had FINISHED when it was written: training resumes at epoch + 1).
    `weight_average`: restored from the checkpoint's two keys when it has them (the caller sees in its `num_updates`
    whether it was); without it the keys are ignored"""
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    model.load_state_dict(model_state_dict(ckpt), strict=True)
    if optimizer is not None and ckpt.get("optimizer_states"):
        optimizer.load_state_dict(ckpt["optimizer_states"][0])
    if scheduler is not None and ckpt.get("lr_schedulers"):
        scheduler.load_state_dict(ckpt["lr_schedulers"][0])
    if weight_average is not None and AVERAGED_KEY in ckpt and AVERAGE_STATE_KEY in ckpt:
        weight_average.load_averaged_state_dict(model_state_dict(ckpt, "averaged"))
        weight_average.load_state_dict(ckpt[AVERAGE_STATE_KEY])
    return ckpt
