"""The gated feed-forward (config key "ff_glu", DESIGN.md §4 "Gated feed-forward") restated for the tests: the gate and its gradient
in float64, the widened weights, and the fp32 step oracle with the MLP line swapped.

    pre = [value | gate]  (columns [0, Hh) and [Hh, 2 Hh))        glu(pre)       = value * act(gate)
    glu_grad(dh, pre) = [dh * act(gate) | dh * value * act'(gate)]               relu'(0) = 0 (the project's h > 0 convention)

act "gelu" is the project's tanh form (tests/gelu_ref.py).  The step composes dalle_step_ref's attention / leaves / gradients and the
oracle's layer_norm / to_logits / loss_fn exactly as dalle_step_ref.forward_logits does and takes the same keywords."""
from collections import OrderedDict

import numpy as np
import torch

import dalle_step_ref as sref
from gelu_ref import gelu, gelu_grad
from loss_weights_ref import weighted_loss_ref
from masked_attention_ref import additive
from oracle import dalle_oracle as do
from token_shift_ref import shift

ACTS = ("relu", "gelu")


def _act(gate, act):
    assert act in ACTS, act
    if act == "gelu":
        return gelu(gate)
    return torch.where(gate > 0, gate, torch.zeros_like(gate)) if torch.is_tensor(gate) else np.where(gate > 0, gate, 0.0)


def _act_grad(gate, act):
    assert act in ACTS, act
    if act == "gelu":
        return gelu_grad(gate)
    return (gate > 0).to(gate.dtype) if torch.is_tensor(gate) else (gate > 0).astype(gate.dtype)


def glu(pre, act):
    """value * act(gate) over the last axis of pre [..., 2 Hh] (numpy or torch, in pre's precision: pass float64)"""
    Hh = pre.shape[-1] // 2
    return pre[..., :Hh] * _act(pre[..., Hh:], act)


def glu_grad(dh, pre, act):
    """d(pre) [..., 2 Hh] from dh [..., Hh]; a zero wherever relu's gate is not positive, whatever dh * value is"""
    Hh = pre.shape[-1] // 2
    val, gate = pre[..., :Hh], pre[..., Hh:]
    dv = dh * _act(gate, act)
    dg = dh * val * _act_grad(gate, act)
    if act == "relu":
        dg = torch.where(gate > 0, dg, torch.zeros_like(dg)) if torch.is_tensor(dg) else np.where(gate > 0, dg, 0.0)
    return torch.cat([dv, dg], -1) if torch.is_tensor(dv) else np.concatenate([dv, dg], -1)


def widen(P0, cfg, seed):
    """P0 with every layer's mlp_linear_1 replaced by seeded [d, 8d] / [8d] arrays: the kernel normal with the reference's stddev
    0.02, the bias the oracle's perturb-style noise N(0, 0.05) so that its gradient is exercised"""
    rng = np.random.default_rng(seed)
    d = cfg.n_embd
    P = OrderedDict((k, v.copy()) for k, v in P0.items())
    for i in range(cfg.n_layers):
        p = f"layer_{i}/mlp/mlp_linear_1/"
        P[p + "kernel"] = (rng.standard_normal((d, 8 * d), dtype=np.float32) * np.float32(0.02)).astype(np.float32)
        P[p + "bias"] = (rng.standard_normal((8 * d,), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    return P


def forward_logits(P, tokens, cfg, *, masks=None, table=None, token_shift=False, dropout=None, activation="relu"):
    """dalle_step_ref.forward_logits with the gated MLP: glu(h @ W1 + b1) @ W2 + b2"""
    assert activation in ACTS, activation
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
        x = x + drop(2 + 2 * i, sref.attention(h, P[p + "attn/q"], P[p + "attn/k"], P[p + "attn/v"], P[p + "attn/o"],
                                               P[p + "attn/compute_output_bias/o_b"], cfg.n_heads,
                                               causal if masks is None else additive(masks[i]), cs))
        h = sh(do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"]))
        w1, b1, w2, b2 = (P[p + "mlp/mlp_linear_" + n] for n in ("1/kernel", "1/bias", "2/kernel", "2/bias"))
        x = x + drop(3 + 2 * i, glu(h @ w1 + b1, activation) @ w2 + b2)
    return do.to_logits(P, x)


def loss_and_grads(params_np, tokens, cfg, *, loss_weights=None, **kw):
    """fp32 (loss, gradients) of the gated model; **kw: forward_logits' keywords"""
    P = sref.leaves(params_np)
    logits = forward_logits(P, tokens, cfg, **kw)
    labels = torch.as_tensor(do.shift_labels(np.asarray(tokens), cfg.eos_token_id), dtype=torch.int64)
    loss, loss_batch = do.loss_fn(logits, labels)
    if loss_weights is not None:
        loss = weighted_loss_ref(loss_batch, cfg.text_seq_len, *loss_weights)[0]
    return float(loss.detach()), sref.gradients(loss, P)
