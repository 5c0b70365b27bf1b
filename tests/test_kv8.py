"""The FP8 key/value cache, CPU side: the format rule of tests/kv8_ref.py (the scaled maximum, both clamps of the exponent, the
error of a dequantised value, exactness in bf16), the oracle with the quantisation removed against dalle_step_ref.forward_logits,
the validation of the argument / flag / config key, and the C ABI's refusals (a status and a message before any launch -- the
pointers below are never dereferenced)."""
import ctypes
import inspect
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dalle_hip as dh  # noqa: E402
import dalle_step_ref as sref  # noqa: E402
import engine_case  # noqa: E402
import kv8_ref  # noqa: E402
from src.dalle_mtf.kv_cache import KV_CACHE_DTYPES, kv_cache_bytes, resolve_kv_cache_dtype  # noqa: E402

FAKE = ctypes.c_void_p(0x10000)
ODD = ctypes.c_void_p(0x10008)
INVALID, UNSUPPORTED = -1, -3


def _rows(seed=0, n=64, hd=128):
    """bf16 rows of every magnitude fp32 products can take, plus the edge rows: one huge, one tiny, all zero, a subnormal maximum"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, hd, generator=g) * torch.exp2(torch.randint(-20, 20, (n, 1), generator=g).float())
    x = x.to(torch.bfloat16)
    x[0] = 0
    x[1] = 0
    x[1, 5] = 3.0e38                      # one huge value: e clamps at 120
    x[2] = 0
    x[2, 7] = -1.0e-38                    # one tiny value (a bf16 subnormal): e clamps at -119
    x[3] = x[3] * 2.0 ** -120             # a row near 2^-126, most of it subnormal
    x[4] = x[4] * 2.0 ** 100
    return x


def test_scaled_maximum_lies_in_128_256_and_the_exponent_clamps():
    x = _rows()
    data, scale = kv8_ref.quantize(x)
    assert data.dtype == torch.uint8 and scale.dtype == torch.float32 and data.shape == x.shape and scale.shape == x.shape[:1]
    e = torch.log2(scale).round().int()
    assert torch.equal(torch.exp2(e.float()), scale)                       # powers of two
    assert int(e.min()) >= -119 and int(e.max()) <= 120
    amax = x.float().abs().amax(-1)
    scaled = amax.double() / scale.double()
    free = (e > -119) & (e < 120) & (amax > 0)
    assert int(free.sum()) > 40
    assert bool(((scaled >= 128) & (scaled < 256))[free].all())
    assert scale[0] == 1.0 and not bool(data[0].any())                     # the all-zero row: e = 0, zeros
    assert e[1] == 120 and 128 <= float(scaled[1]) < 256                   # 3e38 = 1.76 * 2^127
    assert e[2] == -119 and float(scaled[2]) < 128                         # below the clamp the maximum falls short of 128
    assert e[3] == -119
    assert bool((scaled < 256).all())                                      # nothing reaches E4M3's 448, let alone saturates


def test_dequantised_error_and_bf16_exactness():
    x = _rows(seed=1)
    data, scale = kv8_ref.quantize(x)
    y = kv8_ref.dequantize(data, scale)
    assert y.dtype == torch.float32 and torch.equal(y.to(torch.bfloat16).float(), y)       # survives bf16 unchanged
    xd, yd, s = x.double(), y.double(), scale.double()[:, None]
    err = (yd - xd).abs()
    normal = xd.abs() >= s * 2.0 ** -6                                      # E4M3 normals: 3 mantissa bits, half an ulp = 2^-4 relative
    assert bool((err <= 2.0 ** -4 * xd.abs())[normal].all())
    assert bool((err <= (s * 2.0 ** -10).expand_as(err))[~normal].all())    # subnormals: spacing 2^(e - 9)


def test_oracle_without_the_quantisation_is_forward_logits_bit_for_bit():
    cfg, P0, tokens = engine_case.inputs(width=128, heads=2, layers=2, T=8, P=16)
    Pt = {k: torch.tensor(v) for k, v in P0.items()}
    a = sref.forward_logits(Pt, tokens, cfg)
    assert torch.equal(kv8_ref.forward_logits_kv8(Pt, tokens, cfg, kv=None), a)
    b = kv8_ref.forward_logits_kv8(Pt, tokens, cfg)
    assert not torch.equal(a, b) and float((a - b).abs().max() / a.abs().max()) < 0.2


# ---------------------------------------------------------------- argument, flag and config key
def test_kv_cache_dtype_argument_validation():
    assert KV_CACHE_DTYPES == ("bf16", "fp8")
    assert resolve_kv_cache_dtype(None) == "bf16" and resolve_kv_cache_dtype("bf16") == "bf16" and resolve_kv_cache_dtype("fp8") == "fp8"
    for bad in ("int8", "FP8", "", 8, True):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            resolve_kv_cache_dtype(bad)
    with pytest.raises(ValueError, match="kv_cache_dtype.*kv_cache=True"):
        resolve_kv_cache_dtype("fp8", kv_cache=False)
    assert resolve_kv_cache_dtype("bf16", kv_cache=False) == "bf16" and resolve_kv_cache_dtype(None, kv_cache=False) == "bf16"
    from src.dalle_mtf.engine import DalleEngine
    from src.dalle_mtf.models import DALLE
    for fn in (DalleEngine.sample_image_tokens, DALLE.sample):
        assert inspect.signature(fn).parameters["kv_cache_dtype"].default is None
    from src.dalle_mtf.options import Options
    assert "kv_cache_dtype" not in Options._fields                          # a sampler setting, not a model option


def test_cache_bytes_at_the_shipped_predict_batch():
    """dalle_coco (12 layers, width 1024, 8 heads, S = 1280) at B = 128"""
    assert kv_cache_bytes("bf16", 12, 128, 1280, 1024, 8) == 12 * 128 * 1280 * 3 * 1024 * 2 == 12079595520
    assert kv_cache_bytes("fp8", 12, 128, 1280, 1024, 8) == 12 * 128 * 1280 * (2 * 1024 + 8 * 8) == 4152360960


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "generate_dalle.py")] + list(args), cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=120)


def test_generate_cli_flag_and_config_key(tmp_path):
    r = _cli("--help")
    assert r.returncode == 0 and "--kv-cache-dtype" in r.stdout and "{bf16,fp8}" in r.stdout, r.stderr
    r = _cli("--model", "dalle_example", "--from-eval", "2", "--kv-cache-dtype", "int8")
    assert r.returncode == 2 and "--kv-cache-dtype" in r.stderr and "invalid choice" in r.stderr and "Traceback" not in r.stderr
    cfg = json.load(open(os.path.join(ROOT, "configs", "dalle_example.json")))
    bad = tmp_path / "bad.json"
    bad.write_text(json.dumps(dict(cfg, kv_cache_dtype="e5m2")))
    r = _cli("--model", str(bad), "--from-eval", "2")
    assert r.returncode == 2 and "config key kv_cache_dtype" in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
    # the flag goes before the key: with a valid flag the bad key is never consulted, and the next refusal is another argument's
    r = _cli("--model", str(bad), "--from-eval", "2", "--kv-cache-dtype", "fp8", "--top-p", "2")
    assert r.returncode == 2 and "--top-p" in r.stderr and "kv_cache_dtype" not in r.stderr, r.stderr[-2000:]


# ---------------------------------------------------------------- the C ABI refuses bad calls
def _msg():
    return dh.lib().dmi_last_error_string().decode()


def _quant(qkv=FAKE, ld=3 * 256, data=FAKE, scale=FAKE, B=2, S=16, H=2, hd=128, s0=0, s1=16):
    return dh.lib().dmi_kv8_quantize(qkv, ld, data, scale, B, S, H, hd, s0, s1, None)


def _decode(data=FAKE, scale=FAKE, fresh=FAKE, o=FAKE, B=2, H=2, S=16, pos=3, hd=128):
    return dh.lib().dmi_attention_decode_kv8(data, scale, fresh, o, B, H, S, pos, None, hd, None)


def test_entry_points_are_declared_and_bound():
    for name, nargs in (("dmi_kv8_quantize", 11), ("dmi_attention_decode_kv8", 11), ("dmi_attention_decode_kv8_masked", 13)):
        assert name in dh.declared_symbols()
        assert len(getattr(dh.lib(), name).argtypes) == nargs
    assert callable(dh.kv8_quantize) and callable(dh.attention_decode_kv8)


def test_quantiser_refuses_bad_calls_with_a_status_and_a_message():
    assert _quant(qkv=None) == INVALID and "kv8_quantize" in _msg() and "null" in _msg()
    assert _quant(hd=96) == UNSUPPORTED and "head_dim must be 64 or 128" in _msg()
    assert _quant(qkv=ODD) == INVALID and "16-byte aligned" in _msg()
    assert _quant(data=ODD) == INVALID and "16-byte aligned" in _msg()
    for s0, s1 in ((-1, 4), (4, 4), (5, 4), (0, 17), (16, 17)):
        assert _quant(s0=s0, s1=s1) == INVALID and "s0" in _msg(), (s0, s1)
    assert _quant(ld=2 * 256) == INVALID and "ld" in _msg()
    assert _quant(ld=3 * 256 + 4) == INVALID and "ld" in _msg()
    assert _quant(B=0) == INVALID and "empty shape" in _msg()
    with pytest.raises(dh.DalleHipError, match="kv8_quantize"):
        dh._check(_quant(s0=3, s1=2), "kv8_quantize")


def test_decode_refuses_bad_calls_with_a_status_and_a_message():
    assert _decode(fresh=None) == INVALID and "fresh is required" in _msg()
    assert _decode(data=None) == INVALID and "null" in _msg()
    assert _decode(hd=32) == UNSUPPORTED and "attention_decode_kv8" in _msg() and "head_dim" in _msg()
    assert _decode(pos=16) == INVALID and "0 <= pos < S" in _msg()
    assert _decode(pos=-1) == INVALID and "0 <= pos < S" in _msg()
    assert _decode(data=ODD) == INVALID and "16-byte aligned" in _msg()
    assert _decode(B=0) == INVALID and "bad shape" in _msg()
    # a plan with head dim 64 is refused with the masked decode's own message; a buffer that is no plan, too
    from src.dalle_mtf.masks import pattern_mask
    host = np.zeros(64, np.int32)
    L = dh.lib()
    assert L.dmi_attention_decode_kv8_masked(FAKE, FAKE, FAKE, FAKE, FAKE, host.ctypes.data, 2, 2, 16, 3, None, 128, None) == INVALID
    assert "not a mask plan" in _msg()
    m = np.ascontiguousarray(pattern_mask("row", 16, 256))
    n = L.dmi_attn_mask_plan(m.ctypes.data, m.shape[0], None, 0)
    plan = np.zeros(n // 4, np.int32)
    assert L.dmi_attn_mask_plan(m.ctypes.data, m.shape[0], plan.ctypes.data, n) == n
    rc = L.dmi_attention_decode_kv8_masked(FAKE, FAKE, FAKE, FAKE, FAKE, plan.ctypes.data, 2, 2, m.shape[0], 3, None, 64, None)
    assert rc == UNSUPPORTED and "head dim 128" in _msg() and "head dim 64 takes the causal mask only" in _msg()
