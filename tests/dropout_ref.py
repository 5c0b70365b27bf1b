"""numpy restatement of the stateless dropout mask (include/dalle_hip.h "Dropout"; written from the definition, not from
dalle_mtf.dropout) and the fp32 oracle of the DALL-E step with injected per-site masks: oracle.dalle_oracle's attention / mlp /
layer_norm / to_logits / loss_fn composed exactly as its forward_hidden does, every site's tensor multiplied by its 0 / scale mask
where the reference calls mtf.dropout (src/dalle_mtf/models.py:198-200, 215-217, 312-314, 322-323)."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import dalle_oracle as do

U = np.uint64


def splitmix64(x):
    """uint64 array (or scalar) -> uint64, wrapping arithmetic"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U) + U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
        return x ^ (x >> U(31))


def site_key(seed, step, microbatch, rank, site):
    k = splitmix64(U(seed))
    k = splitmix64(k ^ U(step))
    k = splitmix64(k ^ U((microbatch << 32) | rank))
    return int(splitmix64(k ^ U(site)))


def threshold(rate):
    return int(min(max(np.rint(rate * 65536.0), 0), 65535))


def scale(thresh):
    return np.float32(65536.0 / (65536 - thresh))


def keep(key, thresh, n):
    """bool [n]: element e of a site's tensor (row-major) is kept"""
    e = np.arange(n, dtype=U)
    with np.errstate(over="ignore"):
        h = splitmix64(U(key) + (e >> U(2)))
    r = (h >> (U(16) * (e & U(3)))) & U(0xffff)
    return r >= U(thresh)


def mask(key, thresh, shape):
    """float32 array of `shape`: scale where kept, 0 where dropped"""
    n = int(np.prod(shape))
    return np.where(keep(key, thresh, n), scale(thresh), np.float32(0)).astype(np.float32).reshape(shape)


def drop(x32, key, thresh):
    """float32 array -> kept ? x * scale : +0 (one fp32 product)"""
    x32 = np.asarray(x32, np.float32)
    k = keep(key, thresh, x32.size).reshape(x32.shape)
    return np.where(k, x32 * scale(thresh), np.float32(0)).astype(np.float32)


def engine_masks(last_dropout, B, S, d, n_layers):
    """{site: float32 mask} from DalleEngine.last_dropout = {site: (key, thresh)}; a site that is absent is all ones"""
    out = {}
    for site in range(2 + 2 * n_layers):
        shape = (S, d) if site == 1 else (B, S, d)
        out[site] = mask(*last_dropout[site], shape) if site in last_dropout else np.ones(shape, np.float32)
    return out


def loss_and_grads(params_np, tokens, cfg, masks):
    """fp32 loss and every parameter's gradient with the per-site masks of engine_masks (None: no dropout)"""
    P = OrderedDict((n, torch.tensor(a, dtype=torch.float32, requires_grad=True)) for n, a in params_np.items())
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.int64)
    B, S = tok.shape
    one = torch.ones(())
    m = (lambda site: one) if masks is None else (lambda site: torch.from_numpy(masks[site]))
    x = P["embedding/wte"][tok] * m(0) + P["positional_embedding/wpe"][:S] * m(1)
    causal = do.attn_mask(S)
    for i in range(cfg.n_layers):
        p = f"layer_{i}/"
        h = do.layer_norm(x, P[p + "norm_1/g"], P[p + "norm_1/b"])
        x = x + m(2 + 2 * i) * do.attention(h, P[p + "attn/q"], P[p + "attn/k"], P[p + "attn/v"], P[p + "attn/o"],
                                            P[p + "attn/compute_output_bias/o_b"], cfg.n_heads, causal)
        h = do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"])
        x = x + m(3 + 2 * i) * do.mlp(h, P[p + "mlp/mlp_linear_1/kernel"], P[p + "mlp/mlp_linear_1/bias"],
                                      P[p + "mlp/mlp_linear_2/kernel"], P[p + "mlp/mlp_linear_2/bias"])
    logits = do.to_logits(P, x)
    labels = torch.as_tensor(do.shift_labels(np.asarray(tokens), cfg.eos_token_id), dtype=torch.int64)
    loss, _ = do.loss_fn(logits, labels)
    loss.backward()
    grads = OrderedDict((n, p.grad.detach().numpy().copy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32))
                        for n, p in P.items())
    return float(loss.detach()), grads


# ---- the engine-step setup shared by tests/test_dropout.py (CPU: the masks matter here) and tests/test_dropout_gpu.py: the small
# model of tests/test_attn_mask_engine_gpu.py at both widths (n_embd 512 is where the fused LayerNorm products would otherwise run)
T, P, TV, IV, NL, BATCH, RATE = 16, 256, 300, 64, 3, 2, 0.25
WIDTHS = [(256, 2), (512, 4)]


def step_setup(n_embd, n_heads, seed=0):
    cfg = do.DalleConfig(n_embd, TV, IV, T, P, NL, n_heads)
    P0 = do.init_params(cfg, seed=1234 + seed, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(BATCH, T, TV, seed=seed + 1), do.synthetic_image_tokens(BATCH, P, IV, seed=seed + 2), TV)
    return cfg, P0, tokens


def rel_l2(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))
