"""References for token shift (dalle_mtf.token_shift, dmi_token_shift):
  shift64         the float64 shift (or its transpose) of [rows, d] rows, a gather built from shift_sources -- what the kernels
                  are held to, bit for bit;
  shift           the same shift of a torch [B, S, d] tensor, written with slices and pads so that autograd differentiates it;
  loss_and_grads  the fp32 oracle of the DALL-E step with the shift behind both LayerNorms of every block: oracle.dalle_oracle's
                  layer_norm / mlp / to_logits / loss_fn and rotary_ref.attention composed as rotary_ref.forward_logits composes
                  them (table=None: a zero-angle table, which rotates nothing; shift off reproduces
                  oracle.dalle_oracle.loss_and_grads exactly, tests/test_token_shift.py)."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

import rotary_ref as rref
from oracle import dalle_oracle as do
from src.dalle_mtf.token_shift import shift_sources


def shift64(x, T, G, inverse=False):
    """x [rows, d] (any float dtype; rows a multiple of S = T + G * G) -> its float64 shift, or the transpose"""
    x = np.asarray(x, np.float64)
    rows, d = x.shape
    S = T + G * G
    assert rows % S == 0
    src = shift_sources(T, G, d, inverse=inverse)                              # [S, d]
    x3 = x.reshape(rows // S, S, d)
    got = np.take_along_axis(x3, np.broadcast_to(np.maximum(src, 0), x3.shape), axis=1)
    return np.where(src[None] >= 0, got, 0.0).reshape(rows, d)


def shift(x, T, G):
    """x [B, S, d] torch -> shift(x), differentiable: the caption rows move down by one; the image grid moves down by one row for
    the first quarter and right by one column for the second"""
    B, S, d = x.shape
    q = d // 4
    text, img = x[:, :T], x[:, T:].reshape(B, G, G, d)
    text_s = F.pad(text[:, :-1, :2 * q], (0, 0, 1, 0))                         # [B, T, d/2]
    up = F.pad(img[:, :-1, :, :q], (0, 0, 0, 0, 1, 0))                         # from above
    left = F.pad(img[:, :, :-1, q:2 * q], (0, 0, 1, 0))                        # from the left
    img_s = torch.cat([up, left], dim=-1).reshape(B, G * G, 2 * q)
    return torch.cat([torch.cat([text_s, img_s], dim=1), x[:, :, 2 * q:]], dim=-1)


def forward_logits(P, tokens, cfg, table=None, masks=None, token_shift=True):
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.int64)
    S = tok.shape[1]
    T = cfg.text_seq_len
    G = int(round((S - T) ** 0.5))
    assert T + G * G == S
    if table is None:
        table = np.zeros((S, cfg.kv_dim // 2, 2), np.float32)
        table[..., 0] = 1.0
    cs = torch.as_tensor(np.asarray(table), dtype=torch.float32)
    sh = (lambda h: shift(h, T, G)) if token_shift else (lambda h: h)
    x = P["embedding/wte"][tok] + P["positional_embedding/wpe"][:S]
    causal = do.attn_mask(S)
    for i in range(cfg.n_layers):
        p = f"layer_{i}/"
        mask = causal if masks is None else torch.from_numpy(np.where(masks[i], 0.0, -1e10).astype(np.float32))
        h = sh(do.layer_norm(x, P[p + "norm_1/g"], P[p + "norm_1/b"]))
        x = x + rref.attention(h, P[p + "attn/q"], P[p + "attn/k"], P[p + "attn/v"], P[p + "attn/o"],
                               P[p + "attn/compute_output_bias/o_b"], cfg.n_heads, mask, cs)
        h = sh(do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"]))
        x = x + do.mlp(h, P[p + "mlp/mlp_linear_1/kernel"], P[p + "mlp/mlp_linear_1/bias"],
                       P[p + "mlp/mlp_linear_2/kernel"], P[p + "mlp/mlp_linear_2/bias"])
    return do.to_logits(P, x)


def loss_and_grads(params_np, tokens, cfg, table=None, masks=None, token_shift=True):
    """fp32 loss and every parameter's gradient with the shift behind both LayerNorms (token_shift=False: without it); table: an
    optional rotary table [S, head_dim / 2, 2]; masks: optional per-layer bool [S, S] (True = attend), default causal"""
    P = OrderedDict((n, torch.tensor(a, dtype=torch.float32, requires_grad=True)) for n, a in params_np.items())
    logits = forward_logits(P, tokens, cfg, table, masks, token_shift)
    labels = torch.as_tensor(do.shift_labels(np.asarray(tokens), cfg.eos_token_id), dtype=torch.int64)
    loss, _ = do.loss_fn(logits, labels)
    loss.backward()
    grads = OrderedDict((n, p.grad.detach().numpy().copy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                        for n, p in P.items())
    return float(loss.detach()), grads
