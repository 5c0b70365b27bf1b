"""Rotary position embeddings: the config keys "rotary_emb" and "rotary_base" (DESIGN.md §4 "Rotary"; project extensions, the
reference has learned positions only).

Queries and keys are rotated after the QKV projection, pairwise: pair c of a head is its adjacent elements (2c, 2c + 1),
c = 0 .. n - 1, n = head_dim / 2, and at sequence position s
    y0 = x0 cos(a) - x1 sin(a),   y1 = x0 sin(a) + x1 cos(a),   a = angle(s, c).
"1d":    one band of n pairs over the flat position: a = s * base^(-c / n)  (the standard form).
"axial": the pairs are three contiguous bands of n_text = n - 2 (n // 3), n_row = n_col = n // 3 pairs (22 / 21 / 21 at head
         dim 128, 12 / 10 / 10 at 64); pair k of a band of m pairs has frequency base^(-k / m), and the angle is that frequency
         times the band's component of the position triple (text, row, col):
             caption position s < T          -> (s, 0, 0)
             image token k = s - T, grid G   -> (T, 1 + k // G, 1 + k % G)
         so two image tokens moved by the same (row, column) offset keep their q . k.
The learned table positional_embedding/wpe stays: the rotation comes in addition to it.  The key absent, None or False: off --
no table, no launch."""
import math

import numpy as np

SCHEMES = ("1d", "axial")
KEY, BASE_KEY = "rotary_emb", "rotary_base"
DEFAULT_BASE = 10000.0


def grid_side(image_seq_len):
    """G with G * G == image_seq_len, or None"""
    g = math.isqrt(int(image_seq_len))
    return g if g * g == int(image_seq_len) else None


def resolve_rotary(params, image_seq_len=None):
    """(scheme, base) from the config keys: scheme "1d", "axial" or None (key absent, None or False); base a finite number > 1
    (default 10000).  Anything else raises ValueError naming the key; "axial" needs image_seq_len (when given) to be a perfect
    square."""
    params = params or {}
    scheme = params.get(KEY)
    if scheme is None or scheme is False:
        scheme = None
    elif not isinstance(scheme, str) or scheme not in SCHEMES:
        raise ValueError(f"config key {KEY}: expected {' or '.join(map(repr, SCHEMES))}, or null / false for off (got {scheme!r})")
    base = params.get(BASE_KEY)
    base = DEFAULT_BASE if base is None else base
    if isinstance(base, bool) or not isinstance(base, (int, float, np.integer, np.floating)) or not math.isfinite(base) or not base > 1:
        raise ValueError(f"config key {BASE_KEY}: expected a finite number > 1 (got {base!r})")
    if scheme == "axial" and image_seq_len is not None and grid_side(image_seq_len) is None:
        raise ValueError(f"config key {KEY}: 'axial' needs image_seq_len to be a perfect square (got {image_seq_len})")
    return scheme, float(base)


def band_sizes(head_dim):
    """(n_text, n_row, n_col) pairs of the axial bands"""
    n = head_dim // 2
    return n - 2 * (n // 3), n // 3, n // 3


def position_triples(T, P):
    """int64 [T + P, 3]: the (text, row, col) components of every sequence position (axial)"""
    G = grid_side(P)
    if G is None:
        raise ValueError(f"config key {KEY}: 'axial' needs image_seq_len to be a perfect square (got {P})")
    pos = np.zeros((T + P, 3), dtype=np.int64)
    pos[:T, 0] = np.arange(T)
    k = np.arange(P)
    pos[T:, 0], pos[T:, 1], pos[T:, 2] = T, 1 + k // G, 1 + k % G
    return pos


def rotary_angles(scheme, T, P, head_dim, base=DEFAULT_BASE):
    """float64 [S, n]: the angle of pair c at sequence position s"""
    if scheme not in SCHEMES:
        raise ValueError(f"config key {KEY}: expected {' or '.join(map(repr, SCHEMES))} (got {scheme!r})")
    if head_dim % 2:
        raise ValueError(f"rotary embeddings need an even head dim (got {head_dim})")
    n, S = head_dim // 2, T + P
    base = np.float64(base)
    if scheme == "1d":
        return np.arange(S, dtype=np.float64)[:, None] * base ** (-np.arange(n, dtype=np.float64) / n)[None, :]
    pos = position_triples(T, P).astype(np.float64)
    return np.concatenate([pos[:, i:i + 1] * base ** (-np.arange(m, dtype=np.float64) / m)[None, :]
                           for i, m in enumerate(band_sizes(head_dim))], axis=1)


def rotary_table(scheme, T, P, head_dim, base=DEFAULT_BASE):
    """float32 [S, n, 2]: interleaved (cos, sin) of every (position, pair), computed in float64 -- what the engine uploads once"""
    a = rotary_angles(scheme, T, P, head_dim, base)
    return np.stack([np.cos(a), np.sin(a)], axis=-1).astype(np.float32)
