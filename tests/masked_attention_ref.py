"""fp32 oracle of the DALL-E forward with one additive attention mask per layer: oracle.dalle_oracle's attention / mlp /
layer_norm / to_logits / loss_fn composed exactly as its forward_hidden does, with layer l's mask in place of the causal one
(the reference applies attn_mask as the attention bias, src/dalle_mtf/models.py:292-299)."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import dalle_oracle as do


def additive(mask_bool):
    """bool [S, S] (True = attend) -> the reference's additive mask (0 / -1e10)"""
    return torch.from_numpy(np.where(mask_bool, 0.0, -1e10).astype(np.float32))


def loss_and_grads(params_np, tokens, cfg, masks):
    """fp32 loss and every parameter's gradient with per-layer bool masks [S, S]"""
    P = OrderedDict((n, torch.tensor(a, dtype=torch.float32, requires_grad=True)) for n, a in params_np.items())
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.int64)
    S = tok.shape[1]
    x = P["embedding/wte"][tok] + P["positional_embedding/wpe"][:S]
    for i in range(cfg.n_layers):
        p = f"layer_{i}/"
        h = do.layer_norm(x, P[p + "norm_1/g"], P[p + "norm_1/b"])
        x = x + do.attention(h, P[p + "attn/q"], P[p + "attn/k"], P[p + "attn/v"], P[p + "attn/o"],
                             P[p + "attn/compute_output_bias/o_b"], cfg.n_heads, additive(masks[i]))
        h = do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"])
        x = x + do.mlp(h, P[p + "mlp/mlp_linear_1/kernel"], P[p + "mlp/mlp_linear_1/bias"],
                       P[p + "mlp/mlp_linear_2/kernel"], P[p + "mlp/mlp_linear_2/bias"])
    logits = do.to_logits(P, x)
    labels = torch.as_tensor(do.shift_labels(np.asarray(tokens), cfg.eos_token_id), dtype=torch.int64)
    loss, loss_batch = do.loss_fn(logits, labels)
    loss.backward()
    grads = OrderedDict((n, p.grad.detach().numpy().copy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                        for n, p in P.items())
    return float(loss.detach()), loss_batch.detach().numpy(), grads
