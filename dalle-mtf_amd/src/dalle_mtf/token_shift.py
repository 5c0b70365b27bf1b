"""Token shift: the config key "token_shift" (DESIGN.md §4 "Token shift"; a project extension, the reference has none).

Before the attention block and before the feed-forward block of every layer -- behind norm_1 and behind norm_2 -- half of each
position's channels is replaced by the same channels of a neighbour.  With T = text_seq_len, G * G = image_seq_len, d = n_embd,
position p < T a caption position and p >= T image token k = p - T at row r = k // G, column c = k % G, y = shift(x) is

    channels        caption position p < T             image position p >= T
    [0, d/4)        x[p - 1] if p >= 1 else 0          from above:    x[p - G] if r >= 1 else 0
    [d/4, d/2)      x[p - 1] if p >= 1 else 0          from the left: x[p - 1] if c >= 1 else 0
    [d/2, d)        x[p]                               x[p]

so image positions never read caption rows, the first column of an image row does not read the previous row's last column, and
every read is from an earlier position of the same sequence: the shift is causal.  Values are copied, zeros are +0.  The
transpose (dx from dy) is again a gather:

    [0, d/4)        dy[q + 1] if q + 1 < T else 0      dy[q + G] if r + 1 < G else 0
    [d/4, d/2)      dy[q + 1] if q + 1 < T else 0      dy[q + 1] if c + 1 < G else 0
    [d/2, d)        dy[q]                              dy[q]

It has no parameters; it is part of the model (training, evaluation and every sampler), not a regulariser.  The key absent, None
or False: off -- no buffer, no launch.  shift_sources below is the one written-down form of the tables: host code and the tests'
references are built from it."""
import math

import numpy as np

KEY = "token_shift"


def grid_side(image_seq_len):
    """G with G * G == image_seq_len, or None"""
    g = math.isqrt(int(image_seq_len))
    return g if g >= 1 and g * g == int(image_seq_len) else None


def resolve_token_shift(params, n_embd=None, image_seq_len=None):
    """the config key as a bool: absent, None and False are off, True is on; anything else raises ValueError naming the key.  On
    needs image_seq_len (when given) to be a perfect square -- the image tokens' grid -- and n_embd (when given) a multiple of 32:
    each quarter of the channels is then whole 16-byte pieces of bf16."""
    on = (params or {}).get(KEY)
    if on is None or on is False:
        return False
    if on is not True:
        raise ValueError(f"config key {KEY}: expected true, or null / false for off (got {on!r})")
    if image_seq_len is not None and grid_side(image_seq_len) is None:
        raise ValueError(f"config key {KEY}: needs image_seq_len to be a perfect square (got {image_seq_len})")
    if n_embd is not None and (int(n_embd) < 32 or int(n_embd) % 32):
        raise ValueError(f"config key {KEY}: needs n_embd to be a multiple of 32 (got {n_embd})")
    return True


def shift_sources(T, G, d, inverse=False):
    """int64 [T + G * G, d]: the position whose channel ch lands at (position, ch), or -1 for a zero.  inverse: the transpose."""
    T, G, d = int(T), int(G), int(d)
    if T < 1 or G < 1 or d < 4 or d % 4:
        raise ValueError(f"shift_sources: need T >= 1, G >= 1 and d a multiple of 4 (got T={T} G={G} d={d})")
    S = T + G * G
    p = np.arange(S, dtype=np.int64)
    k = p - T
    text = p < T
    r, c = k // G, k % G
    if not inverse:
        prev = np.where(text, p >= 1, c >= 1)
        a = np.where(text, np.where(p >= 1, p - 1, -1), np.where(r >= 1, p - G, -1))     # [0, d/4)
        b = np.where(prev, p - 1, -1)                                                    # [d/4, d/2)
    else:
        nxt = np.where(text, p + 1 < T, c + 1 < G)
        a = np.where(text, np.where(p + 1 < T, p + 1, -1), np.where(r + 1 < G, p + G, -1))
        b = np.where(nxt, p + 1, -1)
    src = np.empty((S, d), dtype=np.int64)
    src[:, :d // 4] = a[:, None]
    src[:, d // 4:d // 2] = b[:, None]
    src[:, d // 2:] = p[:, None]
    return src


def history_bytes(n_layers, batch, seq_len, n_embd):
    """the sampler's shift history: bf16 [B, S, d / 2] for each of the two sites of every layer"""
    return n_layers * 2 * batch * seq_len * (n_embd // 2) * 2
