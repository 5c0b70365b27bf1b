"""CPU reference of the FP8 key/value cache format ("kv8", include/dalle_hip.h): per head row x of head_dim values
    amax = max |x_j|,  e = clamp(floor(log2(amax)) - 7, -119, 120)  (e = 0 when amax = 0),  scale = 2^e,
    data_j = e4m3fn(x_j 2^-e)  -- torch.float8_e4m3fn's round to nearest even of the fp32 product, which is exact for bf16 x.
  quantize(rows)       rows [..., head_dim] (bf16 or fp32) -> (data uint8 [..., head_dim], scale fp32 [...])
  dequantize           float(data) * scale, fp32 -- exact, and exactly representable in bf16 when the rows were
  roundtrip            dequantize(quantize(rows))
  cache_of             the (data [B, S, 2, H, hd], scale [B, S, 2, H]) of a bf16 [B*S, 3 H hd] q | k | v buffer
  forward_logits_kv8   dalle_step_ref.forward_logits (every switch off) with every head's k and v passed through `kv` (default:
                       roundtrip); kv=None gives forward_logits' bits (tests/test_kv8.py)
TEST INFRASTRUCTURE, imported like parity."""
import numpy as np
import torch

from oracle import dalle_oracle as do

E_MIN, E_MAX = -119, 120


def exponent(amax):
    """e of the rule above for a tensor of row maxima (>= 0, finite)"""
    _, ex = torch.frexp(amax.float())                 # amax = m 2^ex, 0.5 <= m < 1: floor(log2(amax)) = ex - 1
    e = (ex.to(torch.int32) - 8).clamp(E_MIN, E_MAX)
    return torch.where(amax > 0, e, torch.zeros_like(e))


def quantize(rows):
    x = rows.float()
    e = exponent(x.abs().amax(-1))
    scaled = torch.ldexp(x, -e[..., None])            # exact: a power of two, and nothing leaves fp32's range
    return scaled.to(torch.float8_e4m3fn).view(torch.uint8), torch.ldexp(torch.ones_like(e, dtype=torch.float32), e)


def dequantize(data, scale):
    return data.view(torch.float8_e4m3fn).float() * scale[..., None]


def roundtrip(rows):
    return dequantize(*quantize(rows))


def cache_of(qkv, B, S, H, hd):
    """qkv bf16 [B*S, 3 H hd] -> the FP8 cache of its k | v columns"""
    return quantize(qkv.detach().cpu().reshape(B, S, 3, H, hd)[:, :, 1:])


def attention(x, wq, wk, wv, wo, o_b, n_heads, mask, kv):
    """dalle_step_ref.attention, k and v of every head through kv"""
    B, S, d = x.shape
    k = d // n_heads
    q = (x @ wq).view(B, S, n_heads, k).transpose(1, 2)
    kk = (x @ wk).view(B, S, n_heads, k).transpose(1, 2)
    v = (x @ wv).view(B, S, n_heads, k).transpose(1, 2)
    if kv is not None:
        kk, v = kv(kk), kv(v)
    logits = q @ kk.transpose(-1, -2)
    logits = logits + mask
    w = torch.exp(logits - torch.logsumexp(logits, dim=-1, keepdim=True))
    a = w @ v
    a = a.transpose(1, 2).reshape(B, S, d)
    return a @ wo + o_b


def forward_logits_kv8(P, tokens, cfg, kv=roundtrip):
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.int64)
    S = tok.shape[1]
    x = P["embedding/wte"][tok] + P["positional_embedding/wpe"][:S]
    causal = do.attn_mask(S)
    for i in range(cfg.n_layers):
        p = f"layer_{i}/"
        h = do.layer_norm(x, P[p + "norm_1/g"], P[p + "norm_1/b"])
        x = x + attention(h, P[p + "attn/q"], P[p + "attn/k"], P[p + "attn/v"], P[p + "attn/o"],
                          P[p + "attn/compute_output_bias/o_b"], cfg.n_heads, causal, kv)
        h = do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"])
        w1, b1, w2, b2 = (P[p + "mlp/mlp_linear_" + n] for n in ("1/kernel", "1/bias", "2/kernel", "2/bias"))
        x = x + do.mlp(h, w1, b1, w2, b2)
    return do.to_logits(P, x)
