"""Text/image loss weights: the config keys "text_loss_weight" and "image_loss_weight" (DESIGN.md §4 "Loss weights").

The reference optimises the plain mean of the cross entropy over all S = T + P positions (src/dalle_mtf/models.py:348-359).
Position p predicts token p + 1 (models.py:407-410): the T - 1 positions p <= T - 2 predict caption tokens, the P + 1 positions
p >= T - 1 predict the image tokens and, the last one, EOS.  With weights (wt, wi) the loss is
    loss = (wt * mean_text(NLL) + wi * mean_image(NLL)) / (wt + wi),
i.e. every position carries a static weight w[p] = wt / ((wt + wi)(T - 1)) or wi / ((wt + wi)(P + 1)) with sum_p w[p] = 1 and
    loss = 1 / (B_global * num_microbatches) * sum_{b,p} w[p] * NLL[b, p].
Both keys absent: the reference's loss, on the kernels it always ran on."""
import math

import numpy as np

KEYS = ("text_loss_weight", "image_loss_weight")


def resolve_loss_weights(params, text_seq_len):
    """(wt, wi) as floats from the two config keys, or None when neither is set (either alone implies 1 for the other).
    Both must be finite and >= 0, not both 0, and text_seq_len >= 2; anything else raises ValueError naming the key."""
    params = params or {}
    given = [params.get(k) for k in KEYS]
    if all(v is None for v in given):
        return None
    out = []
    for k, v in zip(KEYS, given):
        v = 1.0 if v is None else v
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v) or v < 0:
            raise ValueError(f"config key {k}: expected a finite number >= 0 (got {v!r})")
        out.append(float(v))
    if out[0] == 0.0 and out[1] == 0.0:
        raise ValueError(f"config keys {KEYS[0]} and {KEYS[1]}: at least one must be > 0")
    if text_seq_len < 2:
        raise ValueError(f"config keys {KEYS[0]} / {KEYS[1]}: text_seq_len must be >= 2 (got {text_seq_len}): with one caption "
                         "token no position predicts text")
    return out[0], out[1]


def position_weights(text_seq_len, image_seq_len, wt, wi):
    """float64 [T + P]: the static weight of every position (module docstring); the engine uploads it once as fp32."""
    T, P = int(text_seq_len), int(image_seq_len)
    w = np.empty(T + P, np.float64)
    w[:T - 1] = float(wt) / ((float(wt) + float(wi)) * (T - 1))
    w[T - 1:] = float(wi) / ((float(wt) + float(wi)) * (P + 1))
    return w
