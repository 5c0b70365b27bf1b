"""QK normalisation (config key "qk_norm", DESIGN.md §4 "QK norm") restated for the tests:
  qk_norm64 / qk_norm_bwd64   the float64 forward and backward of q | k in the qkv layout, the optional rotation through
                              rotary_ref.rope64 -- what the kernels are held to;
  normalise                   the same normalisation of a torch [B, H, S, k] tensor, differentiable, in the tensor's precision;
  with_gains                  the oracle's weights plus the two gains of every layer, perturbed away from 1;
  forward_logits / loss_and_grads   the fp32 step oracle: dalle_step_ref's leaves, gradients and keywords, its attention restated
                              so that q and k are normalised between the projections and the rotation.

    r(x) = rsqrt(mean_j(x_j^2) + EPS)       q' = q r(q) g_q head_dim^(-1/2)       k' = k r(k) g_k
    dx   = r (a - xh mean_j(a_j xh_j)),  xh = x r(x), a = u dy, u = g c          dg_j = c sum_{rows, heads} dy_j xh_j"""
from collections import OrderedDict

import numpy as np
import torch

import dalle_step_ref as sref
from gelu_ref import gelu
from loss_weights_ref import weighted_loss_ref
from masked_attention_ref import additive
from oracle import dalle_oracle as do
from rotary_ref import rope64, rotate
from token_shift_ref import shift

EPS = 1e-6
GAINS = ("attn/q_norm/g", "attn/k_norm/g")


def _parts(x, gq, gk, H, hd):
    """(x as [rows, 2, H, hd] float64, u = g c as [2, 1, hd], c as [2, 1, 1])"""
    x = np.asarray(x, np.float64)
    c = np.array([float(hd) ** -0.5, 1.0]).reshape(2, 1, 1)
    u = np.stack([np.asarray(gq, np.float64), np.asarray(gk, np.float64)]).reshape(2, 1, hd) * c
    return x[:, :2 * H * hd].reshape(x.shape[0], 2, H, hd), u, c


def qk_norm64(x, gq, gk, H, hd, S=None, cs=None, pos=None):
    """x [rows, ld] (any float dtype) -> float64 copy with columns [0, 2 H hd) normalised and, with cs, rotated (row r at table row
    r % S, or `pos` for every row); the v columns come back unchanged"""
    qk, u, _ = _parts(x, gq, gk, H, hd)
    r = 1.0 / np.sqrt((qk ** 2).mean(-1, keepdims=True) + EPS)
    out = np.asarray(x, np.float64).copy()
    out[:, :2 * H * hd] = (qk * r * u).reshape(out.shape[0], -1)
    return out if cs is None else rope64(out, cs, H, hd, S, pos=pos)


def qk_norm_bwd64(dy, x, gq, gk, H, hd, S=None, cs=None):
    """dy [rows, ld]: the gradient w.r.t. qk_norm64's output; x: its input.  Returns (dx [rows, ld] float64 with the v columns of dy
    unchanged, dgq [hd], dgk [hd], and for the tests' tolerances: the unrotated dy, and sum |terms| of dgq and of dgk)"""
    dy = np.asarray(dy, np.float64)
    if cs is not None:
        dy = rope64(dy, cs, H, hd, S, inverse=True)
    qk, u, c = _parts(x, gq, gk, H, hd)
    d = dy[:, :2 * H * hd].reshape(qk.shape)
    r = 1.0 / np.sqrt((qk ** 2).mean(-1, keepdims=True) + EPS)
    xh = qk * r
    a = u * d
    dx = dy.copy()
    dx[:, :2 * H * hd] = (r * (a - xh * (a * xh).mean(-1, keepdims=True))).reshape(dy.shape[0], -1)
    terms = c * d * xh                                         # [rows, 2, H, hd]
    dg = terms.sum((0, 2))
    mag = np.abs(terms).sum((0, 2))
    return dx, dg[0], dg[1], dy, (mag[0], mag[1])


def normalise(x, g, scale):
    """x [B, H, S, k] torch, g [k]: x r(x) g scale in x's precision (differentiable)"""
    return x * torch.rsqrt((x * x).mean(-1, keepdim=True) + EPS) * g * scale


def with_gains(P0, cfg, seed, noise=0.05):
    """P0 plus every layer's two gains [head_dim] = 1 + N(0, noise): away from 1, so that their gradients and the gains' place in
    dx are exercised (as glu_ref.widen perturbs its bias); noise 0: the initial values, ones"""
    rng = np.random.default_rng(seed)
    hd = cfg.n_embd // cfg.n_heads
    P = OrderedDict((k, v.copy()) for k, v in P0.items())
    for i in range(cfg.n_layers):
        for g in GAINS:
            P[f"layer_{i}/{g}"] = (1.0 + noise * rng.standard_normal(hd)).astype(np.float32)
    return P


def attn_logits(x, wq, wk, gq, gk, n_heads, cs=None):
    """the attention logits [B, H, S, S] before the mask, from normalised (and with cs rotated) q and k; gq None: plain q and k"""
    B, S, d = x.shape
    k = d // n_heads
    q = (x @ wq).view(B, S, n_heads, k).transpose(1, 2)
    kk = (x @ wk).view(B, S, n_heads, k).transpose(1, 2)
    if gq is not None:
        q, kk = normalise(q, gq, float(k) ** -0.5), normalise(kk, gk, 1.0)
    if cs is not None:
        q, kk = rotate(q, cs), rotate(kk, cs)
    return q @ kk.transpose(-1, -2)


def attention(x, wq, wk, wv, wo, o_b, gq, gk, n_heads, mask, cs=None):
    """dalle_step_ref.attention with q and k normalised between the projections and the rotation"""
    B, S, d = x.shape
    k = d // n_heads
    v = (x @ wv).view(B, S, n_heads, k).transpose(1, 2)
    logits = attn_logits(x, wq, wk, gq, gk, n_heads, cs) + mask
    w = torch.exp(logits - torch.logsumexp(logits, dim=-1, keepdim=True))
    a = (w @ v).transpose(1, 2).reshape(B, S, d)
    return a @ wo + o_b


def forward_logits(P, tokens, cfg, *, masks=None, table=None, token_shift=False, dropout=None, activation="relu"):
    """dalle_step_ref.forward_logits with the attention above; the gains come from P"""
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
                                          P[p + "attn/compute_output_bias/o_b"], P[p + GAINS[0]], P[p + GAINS[1]], cfg.n_heads,
                                          causal if masks is None else additive(masks[i]), cs))
        h = sh(do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"]))
        w1, b1, w2, b2 = (P[p + "mlp/mlp_linear_" + n] for n in ("1/kernel", "1/bias", "2/kernel", "2/bias"))
        x = x + drop(3 + 2 * i, do.mlp(h, w1, b1, w2, b2) if activation == "relu" else gelu(h @ w1 + b1) @ w2 + b2)
    return do.to_logits(P, x)


def loss_and_grads(params_np, tokens, cfg, *, loss_weights=None, **kw):
    """fp32 (loss, gradients) of the model with QK normalisation; params_np holds the gains (with_gains); **kw: forward_logits'
    keywords"""
    P = sref.leaves(params_np)
    logits = forward_logits(P, tokens, cfg, **kw)
    labels = torch.as_tensor(do.shift_labels(np.asarray(tokens), cfg.eos_token_id), dtype=torch.int64)
    loss, loss_batch = do.loss_fn(logits, labels)
    if loss_weights is not None:
        loss = weighted_loss_ref(loss_batch, cfg.text_seq_len, *loss_weights)[0]
    return float(loss.detach()), sref.gradients(loss, P)
