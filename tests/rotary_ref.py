"""References for rotary position embeddings (dalle_mtf.rotary, dmi_rope_qk):
  rope64          the float64 rotation of q | k in the qkv layout, from a (cos, sin) table -- what the kernels are held to;
  rotate          the same rotation of a torch [B, H, S, k] tensor, differentiable -- what the fp32 step oracle
                  (tests/dalle_step_ref.py, table=) applies to q and k."""
import numpy as np
import torch


def rope64(x, cs, H, head_dim, S, inverse=False, pos=None):
    """x [rows, ld] (any float dtype) -> float64 copy with columns [0, 2 H head_dim) rotated; row r takes table row r % S (or
    `pos` for every row); cs [S, head_dim / 2, 2].  The v columns come back unchanged."""
    x = np.asarray(x, np.float64)
    rows = x.shape[0]
    n = head_dim // 2
    t = np.asarray(cs, np.float64)[(np.arange(rows) % S) if pos is None else np.full(rows, pos)]     # [rows, n, 2]
    c, s = t[:, None, :, 0], t[:, None, :, 1] * (-1.0 if inverse else 1.0)
    qk = x[:, :2 * H * head_dim].reshape(rows, 2 * H, n, 2)
    y = np.stack([qk[..., 0] * c - qk[..., 1] * s, qk[..., 0] * s + qk[..., 1] * c], axis=-1)
    out = x.copy()
    out[:, :2 * H * head_dim] = y.reshape(rows, -1)
    return out


def rotate(x, cs):
    """x [B, H, S, k] torch fp32, cs [S, k / 2, 2] torch fp32 -> the rotated tensor (fp32, differentiable)"""
    B, H, S, k = x.shape
    p = x.reshape(B, H, S, k // 2, 2)
    c, s = cs[:, :, 0], cs[:, :, 1]
    return torch.stack([p[..., 0] * c - p[..., 1] * s, p[..., 0] * s + p[..., 1] * c], dim=-1).reshape(B, H, S, k)
