"""Embedding and residual dropout: the config keys "embed_dropout", "residual_dropout" and "dropout_seed" (DESIGN.md §4 "Dropout").

The reference drops the token embedding, the positional embedding (src/dalle_mtf/models.py:198-200, 215-217) and the output of
every attention and feed-forward branch before it joins the residual stream (:312-314, 322-323), in training only.  Here a mask
is a pure function of a 64-bit key and the element index (include/dalle_hip.h "Dropout"): element e is kept iff
    (splitmix64(key + (e >> 2)) >> 16 (e & 3)) & 0xffff >= thresh,    thresh = clamp(round(rate * 65536), 0, 65535),
and kept elements are multiplied by fp32(65536 / (65536 - thresh)).  The key of a site depends only on
(seed, optimizer step, microbatch, data-parallel rank, site), so nothing is stored: the re-run of a block under recompute_grad,
the backward and a resumed run restate the same masks.  Both rates absent or 0: no launch changes.
"attention_dropout" stays unsupported (DALLE refuses it)."""
import math

import numpy as np

KEYS = ("embed_dropout", "residual_dropout")
SEED_KEY = "dropout_seed"
MASK64 = (1 << 64) - 1

SITE_TOKEN, SITE_POSITION = 0, 1


def site_attention(layer):
    """the site of layer `layer`'s attention branch (its out-projection output)"""
    return 2 + 2 * layer


def site_mlp(layer):
    """the site of layer `layer`'s feed-forward branch (its second product's output)"""
    return 3 + 2 * layer


def splitmix64(x):
    """the 64-bit finaliser the kernels use (csrc/common.h), on Python ints modulo 2^64"""
    x = (x + 0x9E3779B97F4A7C15) & MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
    return x ^ (x >> 31)


def site_key(seed, step, microbatch, rank, site):
    """sm(sm(sm(sm(seed) ^ step) ^ ((microbatch << 32) | rank)) ^ site), every argument taken modulo 2^64"""
    k = splitmix64(int(seed) & MASK64)
    k = splitmix64(k ^ (int(step) & MASK64))
    k = splitmix64(k ^ ((((int(microbatch) & 0xffffffff) << 32) | (int(rank) & 0xffffffff))))
    return splitmix64(k ^ (int(site) & MASK64))


def threshold(rate):
    """the 16-bit threshold of a rate in [0, 1): clamp(round(rate * 65536), 0, 65535); the effective rate is thresh / 65536"""
    return min(max(int(round(float(rate) * 65536.0)), 0), 65535)


def scale(thresh):
    """what kept elements are multiplied by: 65536 / (65536 - thresh) rounded once to float32 (1.0 at thresh 0)"""
    return np.float32(65536.0 / (65536 - int(thresh)))


def resolve_dropout(params):
    """(embed thresh, residual thresh, seed) from the config keys; a rate that is unset or None counts as 0.  A rate must be a
    finite number in [0, 1), the seed an integer; anything else raises ValueError naming the key."""
    params = params or {}
    out = []
    for k in KEYS:
        v = params.get(k)
        v = 0.0 if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or not (0 <= v < 1):
            raise ValueError(f"config key {k}: expected a finite number in [0, 1) (got {v!r})")
        out.append(threshold(v))
    seed = params.get(SEED_KEY)
    seed = 0 if seed is None else seed
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise ValueError(f"config key {SEED_KEY}: expected an integer (got {seed!r})")
    return out[0], out[1], int(seed)
