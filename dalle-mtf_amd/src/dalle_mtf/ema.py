"""Weight EMA: the config keys "ema_decay" and "ema_eval" (DESIGN.md §4 "Weight EMA").

The reference samples and evaluates the raw iterate of the last optimizer step.  With "ema_decay": d the engine also keeps
tf.train.ExponentialMovingAverage's shadow of every variable,
    ema <- ema - (ema - p) * (1 - decay_t),    decay_t = min(d, (1 + t) / (10 + t))    (TensorFlow's num_updates form),
updated once per optimizer step (t = the 0-based global step of the update), and generation / evaluation can compute from it.
Key absent: no buffer, no launch, the reference's behaviour."""
import math

import numpy as np

KEYS = ("ema_decay", "ema_eval")
WEIGHTS = ("auto", "ema", "raw")


def resolve_ema(params):
    """(decay, ema_eval) from the two config keys.  decay is None when "ema_decay" is unset, None or 0 (off), else a float that
    must be finite with 0 < d < 1; "ema_eval" must be a bool (default False) and needs "ema_decay".  Anything else raises
    ValueError naming the key."""
    params = params or {}
    d, ev = params.get(KEYS[0]), params.get(KEYS[1])
    if d is not None:
        if isinstance(d, bool) or not isinstance(d, (int, float, np.integer, np.floating)) or not math.isfinite(d) \
                or not (0 <= d < 1):
            raise ValueError(f"config key {KEYS[0]}: expected a finite number with 0 < d < 1, or 0 / null for off (got {d!r})")
        d = float(d) or None
    if ev is None:
        ev = False
    if not isinstance(ev, (bool, np.bool_)):
        raise ValueError(f"config key {KEYS[1]}: expected true or false (got {ev!r})")
    if ev and d is None:
        raise ValueError(f"config key {KEYS[1]} needs {KEYS[0]}: there is no average to evaluate")
    return d, bool(ev)


def ema_decay_at(d, t):
    """the decay of the update at 0-based global step t: min(d, (1 + t) / (10 + t)), in Python floats"""
    return min(float(d), (1.0 + t) / (10.0 + t))


def one_minus_decay(d, t):
    """what the kernel is handed: 1 - decay_t rounded once to float32"""
    return float(np.float32(1.0 - ema_decay_at(d, t)))


def resolve_weights(choice, has_ema):
    """"ema" | "raw" from a `weights` argument (None / "auto": the average when there is one); "ema" without one is an error"""
    if choice is None or choice == "auto":
        return "ema" if has_ema else "raw"
    if choice not in ("ema", "raw"):
        raise ValueError(f"weights: expected one of {WEIGHTS} or None (got {choice!r})")
    if choice == "ema" and not has_ema:
        raise ValueError("weights='ema': this model has no weight average (the run sets no ema_decay and its checkpoint carries "
                         "no average)")
    return choice
