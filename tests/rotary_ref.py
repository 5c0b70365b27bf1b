"""References for rotary position embeddings (dalle_mtf.rotary, dmi_rope_qk):
  rope64          the float64 rotation of q | k in the qkv layout, from a (cos, sin) table -- what the kernels are held to;
  loss_and_grads  the fp32 oracle of the DALL-E step with q and k rotated after their projections: oracle.dalle_oracle's
                  layer_norm / mlp / to_logits / loss_fn composed as its forward_hidden does, its attention restated line by
                  line with the rotation between the projections and the logits (an all-zero-angle table reproduces
                  oracle.dalle_oracle.loss_and_grads exactly, tests/test_rotary.py)."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import dalle_oracle as do


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


def attention(x, wq, wk, wv, wo, o_b, n_heads, mask, cs):
    """oracle.dalle_oracle.attention in fp32 (models.py:229-315) with q and k rotated before the logits"""
    B, S, d = x.shape
    k = d // n_heads
    q = (x @ wq).view(B, S, n_heads, k).transpose(1, 2)
    kk = (x @ wk).view(B, S, n_heads, k).transpose(1, 2)
    v = (x @ wv).view(B, S, n_heads, k).transpose(1, 2)
    q, kk = rotate(q, cs), rotate(kk, cs)
    logits = q @ kk.transpose(-1, -2)
    logits = logits + mask
    w = torch.exp(logits - torch.logsumexp(logits, dim=-1, keepdim=True))
    a = w @ v
    a = a.transpose(1, 2).reshape(B, S, d)
    return a @ wo + o_b


def forward_logits(P, tokens, cfg, table, masks=None):
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.int64)
    S = tok.shape[1]
    cs = torch.as_tensor(np.asarray(table), dtype=torch.float32)
    x = P["embedding/wte"][tok] + P["positional_embedding/wpe"][:S]
    causal = do.attn_mask(S)
    for i in range(cfg.n_layers):
        p = f"layer_{i}/"
        mask = causal if masks is None else torch.from_numpy(np.where(masks[i], 0.0, -1e10).astype(np.float32))
        h = do.layer_norm(x, P[p + "norm_1/g"], P[p + "norm_1/b"])
        x = x + attention(h, P[p + "attn/q"], P[p + "attn/k"], P[p + "attn/v"], P[p + "attn/o"],
                          P[p + "attn/compute_output_bias/o_b"], cfg.n_heads, mask, cs)
        h = do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"])
        x = x + do.mlp(h, P[p + "mlp/mlp_linear_1/kernel"], P[p + "mlp/mlp_linear_1/bias"],
                       P[p + "mlp/mlp_linear_2/kernel"], P[p + "mlp/mlp_linear_2/bias"])
    return do.to_logits(P, x)


def loss_and_grads(params_np, tokens, cfg, table, masks=None):
    """fp32 loss and every parameter's gradient with q, k rotated by `table` [S, head_dim / 2, 2]; masks: optional per-layer bool
    [S, S] (True = attend), default causal"""
    P = OrderedDict((n, torch.tensor(a, dtype=torch.float32, requires_grad=True)) for n, a in params_np.items())
    logits = forward_logits(P, tokens, cfg, table, masks)
    labels = torch.as_tensor(do.shift_labels(np.asarray(tokens), cfg.eos_token_id), dtype=torch.int64)
    loss, _ = do.loss_fn(logits, labels)
    loss.backward()
    grads = OrderedDict((n, p.grad.detach().numpy().copy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                        for n, p in P.items())
    return float(loss.detach()), grads
