"""Named attention-mask patterns for DALLE(attn_mask=...) and the "attention_pattern" config key (DESIGN.md §4 "Attention masks").

A mask is a boolean [S, S] array, S = text length T + image length P; M[i, j] means "query i may attend to key j".  Text queries are
always plain causal.  An image query i at grid cell (r, c) of the W x W image grid (W = sqrt(P)) sees every text key, itself, and
the image keys j <= i the pattern selects:
  causal     all of them (the reference's mask; the default)
  local:R    i - j <= R: a sliding window over the flattened image.  This is NOT mesh-tensorflow's blocked local_attention_1d.
  row        the same grid row
  column     the same grid column
  conv:K     K odd: rows r-K+1 .. r and columns |c' - c| <= (K-1)/2
Every pattern is causal and leaves no row empty, so the attention kernels accept it."""
import math

import numpy as np

PATTERNS = ("causal", "local:R", "row", "column", "conv:K")


def _grid_width(image_len, name):
    w = math.isqrt(image_len)
    if w * w != image_len:
        raise ValueError(f"attention pattern {name!r} needs a square image grid (image_seq_len = {image_len} is not a perfect square)")
    return w


def pattern_mask(name, text_len, image_len):
    """dense bool [S, S] mask of a named pattern (see the module docstring)"""
    if not isinstance(name, str):
        raise TypeError(f"attention pattern must be a string (got {type(name).__name__})")
    T, P = int(text_len), int(image_len)
    S = T + P
    causal = np.tril(np.ones((S, S), dtype=bool))
    kind, _, arg = name.partition(":")
    if kind == "causal" and not arg:
        return causal
    ii = np.arange(P)[:, None]   # image query index
    jj = np.arange(P)[None, :]   # image key index
    if kind == "local":
        try:
            R = int(arg)
        except ValueError:
            R = -1
        if R < 0:
            raise ValueError(f"attention pattern {name!r}: local:R needs an integer R >= 0")
        img = (ii - jj) <= R
    elif kind in ("row", "column", "conv"):
        W = _grid_width(P, name)
        ri, ci, rj, cj = ii // W, ii % W, jj // W, jj % W
        if kind == "row" and not arg:
            img = ri == rj
        elif kind == "column" and not arg:
            img = ci == cj
        elif kind == "conv":
            try:
                K = int(arg)
            except ValueError:
                K = 0
            if K < 1 or K % 2 == 0:
                raise ValueError(f"attention pattern {name!r}: conv:K needs an odd integer K >= 1")
            img = (ri - rj <= K - 1) & (np.abs(cj - ci) <= (K - 1) // 2)
        else:
            raise ValueError(f"unknown attention pattern {name!r} (known: {', '.join(PATTERNS)})")
    else:
        raise ValueError(f"unknown attention pattern {name!r} (known: {', '.join(PATTERNS)})")
    m = causal.copy()
    m[T:, T:] &= img | (ii == jj)
    return m


def check_mask(m, S, what="attn_mask"):
    """validate a dense bool mask: shape [S, S], causal, no empty row"""
    if m.shape != (S, S):
        raise ValueError(f"{what}: expected shape [{S}, {S}], got {list(m.shape)}")
    if np.triu(m, 1).any():
        i, j = np.argwhere(np.triu(m, 1))[0]
        raise ValueError(f"{what}: the mask is not causal (query {i} attends to key {j}); it could not be sampled autoregressively")
    empty = np.flatnonzero(~m.any(axis=1))
    if empty.size:
        raise ValueError(f"{what}: query {empty[0]} attends to no key (every row needs at least one allowed key)")
    return m


def to_bool_mask(spec, text_len, image_len, what="attn_mask"):
    """one layer's mask from a pattern string, a bool [S, S] array / tensor, or an additive float mask (0 or <= -1e9, the reference's
    convention) -> validated bool numpy [S, S]"""
    S = int(text_len) + int(image_len)
    if isinstance(spec, str):
        return pattern_mask(spec, text_len, image_len)
    a = spec.detach().cpu().numpy() if hasattr(spec, "detach") else np.asarray(spec)
    if a.dtype == bool:
        m = a
    elif np.issubdtype(a.dtype, np.floating):
        ok = (a == 0) | (a <= -1e9)
        if not ok.all():
            raise ValueError(f"{what}: an additive float mask must hold 0 (attend) or values <= -1e9 (masked); found {a[~ok].flat[0]!r}")
        m = a == 0
    else:
        raise TypeError(f"{what}: expected a pattern string, a bool mask or an additive float mask (got dtype {a.dtype})")
    return check_mask(np.ascontiguousarray(m, dtype=bool), S, what)


def layer_masks(spec, n_layers, text_len, image_len):
    """per-layer bool masks from DALLE(attn_mask=...) / "attention_pattern": one spec for every layer, or a list of exactly n_layers"""
    if isinstance(spec, (list, tuple)):
        if len(spec) != n_layers:
            raise ValueError(f"attn_mask: a per-layer list needs exactly n_layers = {n_layers} entries (got {len(spec)})")
        return [to_bool_mask(s, text_len, image_len, f"attn_mask[{i}]") for i, s in enumerate(spec)]
    m = to_bool_mask(spec, text_len, image_len)
    return [m] * n_layers
