"""The sampler's key/value cache type: a sampler setting (DalleEngine.sample_image_tokens(kv_cache_dtype=...), generate_dalle.py
--kv-cache-dtype, the config key "kv_cache_dtype"), not a model option -- checkpoints do not record it.
  "bf16"  the [B*S, 3d] projection buffers of the forward pass (the default)
  "fp8"   K and V in OCP E4M3 with one power-of-two scale per (position, head): DESIGN.md §4 "Generation: FP8 key/value cache"
Pure host code."""

KV_CACHE_DTYPES = ("bf16", "fp8")
DEFAULT = "bf16"


def resolve_kv_cache_dtype(kv_cache_dtype, kv_cache=True):
    """the cache type of a sampling call: None is the default ("bf16"); anything but a member of KV_CACHE_DTYPES, or "fp8" without
    the cache itself, is a ValueError naming the argument"""
    if kv_cache_dtype is None:
        return DEFAULT
    if not isinstance(kv_cache_dtype, str) or kv_cache_dtype not in KV_CACHE_DTYPES:
        raise ValueError(f"kv_cache_dtype must be one of {KV_CACHE_DTYPES} or None (got {kv_cache_dtype!r})")
    if kv_cache_dtype == "fp8" and not kv_cache:
        raise ValueError("kv_cache_dtype='fp8' needs kv_cache=True: without the cache every position is a full forward")
    return kv_cache_dtype


def kv_cache_bytes(kv_cache_dtype, n_layers, batch, seq_len, n_embd, n_heads):
    """bytes of the per-layer caches: bf16 keeps q | k | v rows (L B S 3d 2), fp8 a byte per k, v element and two fp32 scales per
    (position, head) (L B S (2d + 8H))"""
    per_pos = 3 * n_embd * 2 if resolve_kv_cache_dtype(kv_cache_dtype) == "bf16" else 2 * n_embd + 8 * n_heads
    return n_layers * batch * seq_len * per_pos
