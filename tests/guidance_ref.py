"""numpy float32 restatement of the guided logits of dmi_sample_tokens_guided (include/dalle_hip.h), in the kernel's rounding
order: d = zc - zu, t = (scale - 1) * d, g = zc + t, each a float32 operation of its own (no fused multiply-add), and g = zc
itself when scale - 1 == 0.  The kept set is nucleus_ref.nucleus_keep over g * (1/temperature)."""
import numpy as np

from nucleus_ref import nucleus_keep


def guided_logits(zc, zu, scale):
    """zc, zu: float32 [..., nv], already z + bias.  Returns g float32, bit for bit what the kernel filters and draws from."""
    zc = np.asarray(zc, np.float32)
    zu = np.asarray(zu, np.float32)
    sm1 = np.float32(scale) - np.float32(1)
    if sm1 == 0:
        return zc.copy()
    d = (zc - zu).astype(np.float32)
    t = (sm1 * d).astype(np.float32)
    return (zc + t).astype(np.float32)


def scaled(g, temperature):
    """v = g * (1/temperature) as the kernel forms it: one float32 reciprocal, one float32 product"""
    return (np.asarray(g, np.float32) * (np.float32(1) / np.float32(temperature))).astype(np.float32)


def guided_keep(zc, zu, scale, temperature, top_k=0, top_p=1.0):
    """bool mask of the entries a guided draw may return for one pair of rows"""
    return nucleus_keep(scaled(guided_logits(zc, zu, scale), temperature), top_k, top_p)
