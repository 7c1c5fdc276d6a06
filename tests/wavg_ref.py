"""numpy float32 restatements of the weight-averaging updates (lidog_amd/csrc/wavg.hip, lidog_amd.optim.WeightAverage):
every operation is one float32 operation, rounded on its own, in the order the kernel states it.  No torch."""
import math

import numpy as np

F32 = np.float32


def tau(s, decay, final_decay=None, total_steps=None):
    """the decay of the update after `s` earlier ones: constant, or the cosine schedule from `decay` to `final_decay`
    over `total_steps` updates (python doubles)"""
    if final_decay is None:
        return decay
    return final_decay - (final_decay - decay) * (math.cos(math.pi * s / total_steps) + 1) / 2


def ema_step(a, p, t):
    """a' = c0 * a + c1 * p with c0 = float32(t), c1 = float32(1 - t), the subtraction in double"""
    c0, c1 = F32(t), F32(1.0 - t)
    a, p = np.asarray(a, dtype=F32), np.asarray(p, dtype=F32)
    return ((c0 * a).astype(F32) + (c1 * p).astype(F32)).astype(F32)


def swa_step(a, p, n):
    """a' = a + (p - a) / (n + 1) after `n` earlier updates"""
    a, p = np.asarray(a, dtype=F32), np.asarray(p, dtype=F32)
    d = (p - a).astype(F32)
    return (a + (d / F32(n + 1)).astype(F32)).astype(F32)


def update(a, p, s, mode, decay=0.996, final_decay=None, total_steps=None):
    """the average after the update that follows `s` earlier ones: a copy first, then the mode's step"""
    if s == 0:
        return np.array(p, dtype=F32, copy=True)
    if mode == "ema":
        return ema_step(a, p, tau(s, decay, final_decay, total_steps))
    return swa_step(a, p, s)
