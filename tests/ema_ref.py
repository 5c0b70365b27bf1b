"""numpy restatement of the weight EMA (include/dalle_hip.h dmi_ema_step, DESIGN.md §4 "Weight EMA"); no project imports.

ema <- ema - (ema - p) * one_minus_decay in float32: the difference, the product and the second difference are three float32
operations, each rounded on its own (numpy never fuses them).  The bf16 copy is rounded to nearest even from the float32 result."""
import numpy as np


def ema_step_ref(ema, p, omd):
    ema, p, omd = np.asarray(ema, np.float32), np.asarray(p, np.float32), np.float32(omd)
    with np.errstate(all="ignore"):
        d = (ema - p).astype(np.float32)
        t = (d * omd).astype(np.float32)
        return (ema - t).astype(np.float32)


def bf16_rne_bits(x):
    """uint16 bfloat16 bits of float32 x, round to nearest even; NaN stays NaN (quiet bit set, as hardware conversions do)"""
    u = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    r = ((u.astype(np.uint64) + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(np.asarray(x, np.float32))
    return np.where(nan, ((u >> 16) | 0x40).astype(np.uint16), r)


def bf16_to_f32(bits):
    return (np.asarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32)


def ema_decay_at(d, t):
    """TensorFlow's num_updates form: min(d, (1 + t) / (10 + t)), t the 0-based step of the update, Python floats"""
    return min(float(d), (1.0 + t) / (10.0 + t))


def one_minus_decay(d, t):
    return float(np.float32(1.0 - ema_decay_at(d, t)))
