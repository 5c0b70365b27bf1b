"""The fp32 oracle of the DALL-E step with every option of the engine behind a keyword: oracle.dalle_oracle's layer_norm / attn_mask /
mlp / to_logits / loss_fn / shift_labels composed exactly as its forward_hidden composes them, its attention restated once in fp32
(the rotation of q and k goes between the projections and the logits).  With every switch off the torch operations, and their
order, are those of oracle.dalle_oracle.loss_and_grads(bf16=False): same loss, same gradients, bit for bit
(tests/test_step_ref.py).  fp32 only; the bf16 and teacher-forcing modes stay in oracle/dalle_oracle.py.
  masks        per-layer bool [S, S], True = attend (the reference applies attn_mask as the attention bias,
               src/dalle_mtf/models.py:292-299); None: causal
  table        rotary (cos, sin) table [S, head_dim / 2, 2]; None: no rotation at all
  token_shift  token_shift_ref.shift behind both LayerNorms of every block
  dropout      {site: float32 0 / scale mask} of dropout_ref.engine_masks, multiplied in where the reference calls mtf.dropout
               (src/dalle_mtf/models.py:198-200, 215-217, 312-314, 322-323); None: no multiply
  activation   "relu" or "gelu" (gelu_ref.gelu in the feed-forward, src/dalle_mtf/models.py:317-324)
  loss_weights (text, image) through loss_weights_ref.weighted_loss_ref; None: the reference's mean over all positions"""
from collections import OrderedDict

import numpy as np
import torch

from gelu_ref import gelu
from loss_weights_ref import weighted_loss_ref
from masked_attention_ref import additive
from oracle import dalle_oracle as do
from rotary_ref import rotate
from token_shift_ref import shift


def attention(x, wq, wk, wv, wo, o_b, n_heads, mask, cs=None):
    """oracle.dalle_oracle.attention in fp32 (models.py:229-315); cs: q and k rotated before the logits"""
    B, S, d = x.shape
    k = d // n_heads
    q = (x @ wq).view(B, S, n_heads, k).transpose(1, 2)
    kk = (x @ wk).view(B, S, n_heads, k).transpose(1, 2)
    v = (x @ wv).view(B, S, n_heads, k).transpose(1, 2)
    if cs is not None:
        q, kk = rotate(q, cs), rotate(kk, cs)
    logits = q @ kk.transpose(-1, -2)
    logits = logits + mask
    w = torch.exp(logits - torch.logsumexp(logits, dim=-1, keepdim=True))
    a = w @ v
    a = a.transpose(1, 2).reshape(B, S, d)
    return a @ wo + o_b


def forward_logits(P, tokens, cfg, *, masks=None, table=None, token_shift=False, dropout=None, activation="relu"):
    assert activation in ("relu", "gelu"), activation
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.int64)
    S = tok.shape[1]
    T = cfg.text_seq_len
    G = int(round((S - T) ** 0.5))
    cs = None if table is None else torch.as_tensor(np.asarray(table), dtype=torch.float32)
    sh = (lambda h: shift(h, T, G)) if token_shift else (lambda h: h)
    drop = (lambda site, t: t) if dropout is None else (lambda site, t: torch.from_numpy(dropout[site]) * t)
    x = drop(0, P["embedding/wte"][tok]) + drop(1, P["positional_embedding/wpe"][:S])
    causal = do.attn_mask(S)
    for i in range(cfg.n_layers):
        p = f"layer_{i}/"
        h = sh(do.layer_norm(x, P[p + "norm_1/g"], P[p + "norm_1/b"]))
        x = x + drop(2 + 2 * i, attention(h, P[p + "attn/q"], P[p + "attn/k"], P[p + "attn/v"], P[p + "attn/o"],
                                          P[p + "attn/compute_output_bias/o_b"], cfg.n_heads,
                                          causal if masks is None else additive(masks[i]), cs))
        h = sh(do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"]))
        w1, b1, w2, b2 = (P[p + "mlp/mlp_linear_" + n] for n in ("1/kernel", "1/bias", "2/kernel", "2/bias"))
        x = x + drop(3 + 2 * i, do.mlp(h, w1, b1, w2, b2) if activation == "relu" else gelu(h @ w1 + b1) @ w2 + b2)
    return do.to_logits(P, x)


def leaves(params_np):
    """the parameters as fp32 autograd leaves, under the reference's names"""
    return OrderedDict((n, torch.tensor(a, dtype=torch.float32, requires_grad=True)) for n, a in params_np.items())


def forward_loss(P, tokens, cfg, **kw):
    """(the reference's loss, loss_batch [B, S]) of one forward; **kw: forward_logits' keywords"""
    logits = forward_logits(P, tokens, cfg, **kw)
    labels = torch.as_tensor(do.shift_labels(np.asarray(tokens), cfg.eos_token_id), dtype=torch.int64)
    return do.loss_fn(logits, labels)


def gradients(loss, P, retain_graph=False):
    """every parameter's gradient of `loss` as numpy, zeros for a parameter the loss does not reach"""
    g = torch.autograd.grad(loss, list(P.values()), retain_graph=retain_graph, allow_unused=True)
    return OrderedDict((n, x.numpy().copy() if x is not None else np.zeros(tuple(p.shape), np.float32))
                       for (n, p), x in zip(P.items(), g))


def loss_and_grads(params_np, tokens, cfg, *, loss_weights=None, **kw):
    """fp32 (loss, gradients); **kw: forward_logits' keywords"""
    P = leaves(params_np)
    loss, loss_batch = forward_loss(P, tokens, cfg, **kw)
    if loss_weights is not None:
        loss = weighted_loss_ref(loss_batch, cfg.text_seq_len, *loss_weights)[0]
    return float(loss.detach()), gradients(loss, P)
