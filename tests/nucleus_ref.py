"""numpy restatement of the nucleus set of dmi_sample_tokens_p (include/dalle_hip.h): the top-k filter with ties of the k-th value
kept, then q quantised to u = floor(exp(v - max v) * 2^31) over the survivors, the mass a 64-bit integer sum, the target
ceil(double(top_p) * Z), and every survivor with u >= tau kept, tau the u of the last entry of the shortest descending prefix
that reaches the target."""
import math

import numpy as np


def topk_keep(v, top_k):
    v = np.asarray(v, np.float32)
    if 0 < top_k < v.shape[0]:
        return v >= np.sort(v)[::-1][top_k - 1]
    return np.ones(v.shape[0], bool)


def quantised_q(v, keep):
    v = np.asarray(v, np.float32)
    e = np.exp(v - v.max()).astype(np.float32)
    return np.where(keep, np.floor(e.astype(np.float64) * 2.0 ** 31), 0).astype(np.uint64)


def nucleus_keep(v, top_k=0, top_p=1.0):
    """v: float32 [nv], already (z + bias) / temperature.  Returns the kept set as a bool mask."""
    keep = topk_keep(v, top_k)
    if not (0.0 < top_p < 1.0):
        return keep
    u = quantised_q(v, keep)
    mass = int(u.sum())
    target = math.ceil(float(np.float32(top_p)) * float(mass))
    us = np.sort(u)[::-1]
    tau = us[int(np.argmax(np.cumsum(us) >= target))]
    return keep & (u >= tau)
