"""The FP8 key/value cache through the engine, the samplers and the command line on the GPU, on the engine_case model (T 16, P 256,
3 layers) at width 256 (two heads of 128) and 128 (two heads of 64).

Exact: after an fp8 prefill every layer's cache is tests/kv8_ref.py's quantisation of the k | v columns of that layer's projection
buffer, and after the teacher-forced decode of every image position layer 0's rows are the quantisation of the rows the bf16-cache
engine wrote (layer 0's k and v do not depend on attention).  Paths: the three samplers agree, completion returns the sample, a
recompute_grad engine draws the same tokens without ever allocating the bf16 caches, and bf16 sampling is untouched by an fp8 call
before it.  The logits get a sanity bound only (test_decode_logits_sanity_bound)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import engine_case
import kv8_ref
from engine_case import IV, T, TV

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = [256, 128]
_RUNS = {}


def _run(width):
    """one engine per width, and what every test of it shares: the bf16 and the fp8 teacher-forced decode of every image position
    (logits [B, P, IV] each), layer 0's bf16 rows after the former, the fp8 caches after the prefill and after the decode"""
    if width not in _RUNS:
        cfg, model, P0, tokens = engine_case.build(width=width)
        eng = model.engine
        tok = torch.from_numpy(tokens).cuda()
        r = dict(cfg=cfg, eng=eng, P0=P0, tokens=tokens, tok=tok)
        for kv in ("bf16", "fp8"):
            with eng.kv_cache_as(kv):
                eng._prefill(tok)
                if kv == "fp8":
                    r["qkv_prefill"] = [t.cpu() for t in eng.qkv]
                    r["kv8_prefill"] = [(d.cpu(), s.cpu()) for d, s in eng._kv8]
                z = [eng.decode_step(tok[:, pos].contiguous(), pos, graph=True).clone() for pos in range(eng.T - 1, eng.S - 1)]
                r["z_" + kv] = torch.stack(z, 1).cpu()
            if kv == "bf16":
                r["qkv0_bf16"] = eng.qkv[0].cpu()
            else:
                r["kv8_decode0"] = tuple(t.cpu() for t in eng._kv8[0])
        _RUNS[width] = r
    return _RUNS[width]


def _same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


@pytest.mark.parametrize("width", WIDTHS)
def test_prefill_quantises_every_layers_rows_exactly(width):
    r = _run(width)
    eng = r["eng"]
    assert not eng.recompute and len(r["kv8_prefill"]) == eng.L
    for l in range(eng.L):
        data, scale = r["kv8_prefill"][l]
        assert data.shape == (eng.B, eng.S, 2, eng.H, eng.hd) and scale.shape == (eng.B, eng.S, 2, eng.H)
        assert _same((data, scale), kv8_ref.cache_of(r["qkv_prefill"][l], eng.B, eng.S, eng.H, eng.hd)), f"layer {l}"


@pytest.mark.parametrize("width", WIDTHS)
def test_decode_writes_layer0_rows_of_the_bf16_engine_quantised(width):
    r = _run(width)
    eng = r["eng"]
    want = kv8_ref.cache_of(r["qkv0_bf16"], eng.B, eng.S, eng.H, eng.hd)
    rows = slice(eng.T - 1, eng.S - 1)                     # the decoded positions; the others are the prefill's
    assert _same(tuple(t[:, rows] for t in r["kv8_decode0"]), tuple(t[:, rows] for t in want))
    keep = [i for i in range(eng.S) if not (eng.T - 1 <= i < eng.S - 1)]
    assert _same(tuple(t[:, keep] for t in r["kv8_decode0"]), tuple(t[:, keep] for t in r["kv8_prefill"][0]))


def _err(z, ref):
    """engine_case.decode_worst's statistic: the worst max |z - ref| / max |ref| over the image positions; z, ref [B, P, IV]"""
    return max(float((z[:, i] - ref[:, i]).abs().max() / ref[:, i].abs().max()) for i in range(z.shape[1]))


@pytest.mark.parametrize("width", WIDTHS)
def test_decode_logits_sanity_bound(width):
    """err8 <= E16 + Dq, all three the statistic of engine_case.decode_worst against CPU fp32 references:
      err8  the fp8-cache engine's decode logits against kv8_ref.forward_logits_kv8
      E16   the bf16-cache engine's decode logits against dalle_step_ref.forward_logits
      Dq    forward_logits_kv8 against forward_logits: what the quantisation itself moves
    A sanity bound, wide on purpose: bf16 noise in k and v flips FP8 roundings, which alone moves the CPU logits by about half of
    Dq, so no tight comparison against a CPU model is possible; the exact checks above carry correctness, this one catches a
    wrong layer, head or scale, which moves the logits by far more than Dq.
    Measured on an MI355X (the test prints them as a KV8 LOGITS line):
      width 256 (head dim 128): err8 0.0426  E16 0.0114  Dq 0.0534
      width 128 (head dim 64):  err8 0.0251  E16 0.0138  Dq 0.0294"""
    import dalle_step_ref as sref
    r = _run(width)
    eng = r["eng"]
    Pt = {k: torch.tensor(v) for k, v in r["P0"].items()}
    pos = slice(eng.T - 1, eng.S - 1)
    ref = sref.forward_logits(Pt, r["tokens"], r["cfg"])[:, pos, TV:TV + IV]
    ref8 = kv8_ref.forward_logits_kv8(Pt, r["tokens"], r["cfg"])[:, pos, TV:TV + IV]
    err8, E16, Dq = _err(r["z_fp8"], ref8), _err(r["z_bf16"], ref), _err(ref8, ref)
    print(f"KV8 LOGITS width {width}: err8 {err8:.4g}  E16 {E16:.4g}  Dq {Dq:.4g}", flush=True)
    assert err8 <= E16 + Dq, (err8, E16, Dq)


@pytest.mark.parametrize("width", WIDTHS)
def test_samplers_agree_and_completion_returns_the_sample(width):
    r = _run(width)
    eng = r["eng"]
    text = r["tok"][:, :T].contiguous()
    with eng.kv_cache_as("fp8"):
        engine_case.samplers_agree(eng, text)
    kw = dict(temperature=1.0, top_k=8, seed=3, kv_cache_dtype="fp8")
    s = eng.sample_image_tokens(text, **kw)
    assert eng.kv_cache_dtype == "bf16" and any(isinstance(k, tuple) and k[0] == "fp8" for k in eng._dec["graphs"])
    for k in (1, 17):
        assert torch.equal(eng.sample_image_tokens(text, image_prefix=s[:, :k].cpu(), **kw), s), k
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        eng.sample_image_tokens(text, kv_cache_dtype="int8")
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        eng.sample_image_tokens(text, kv_cache_dtype="fp8", kv_cache=False)


def test_recompute_engine_samples_the_same_tokens_without_bf16_caches():
    r = _run(256)
    text = r["tok"][:, :T].contiguous()
    kw = dict(temperature=1.0, top_k=8, seed=3, top_p=0.9, return_logprobs=True, kv_cache_dtype="fp8")
    a, lp = r["eng"].sample_image_tokens(text, **kw)
    _, model, _, _ = engine_case.build(width=256, hparams=dict(recompute_grad=True))
    eng = model.engine
    assert eng.recompute
    b, lpb = eng.sample_image_tokens(text, **kw)
    assert torch.equal(a, b) and torch.equal(lp, lpb)
    assert eng._kv is None and len(eng._kv8) == eng.L
    ptrs = [d.data_ptr() for d, _ in eng._kv8]
    eng.sample_image_tokens(text, **kw)
    assert eng._kv is None and [d.data_ptr() for d, _ in eng._kv8] == ptrs      # allocated once and kept


@pytest.mark.parametrize("first", ["fp8", "bf16"])
def test_bf16_tokens_do_not_depend_on_fp8_calls(first):
    r = _run(256)
    text = r["tok"][:, :T].contiguous()
    kw = dict(temperature=1.0, top_k=8, seed=7)
    _, model, _, _ = engine_case.build(width=256)
    fresh = model.engine.sample_image_tokens(text, **kw)                       # an engine that never saw fp8
    assert model.engine._kv8 is None
    del model
    _, model, _, _ = engine_case.build(width=256)
    eng = model.engine
    out = {}
    for kv in (first, "fp8" if first == "bf16" else "bf16"):
        out[kv] = eng.sample_image_tokens(text, kv_cache_dtype=kv, **kw)
    assert torch.equal(out["bf16"], fresh)
    assert torch.equal(eng.sample_image_tokens(text, **kw), fresh)             # and again, on the captured bf16 graph


def test_generate_cli_with_the_flag(tmp_path):
    """--kv-cache-dtype fp8 end to end in a fresh child process; the flag goes before the config key; generate.json records it"""
    vae = json.load(open(os.path.join(ROOT, "configs", "vae_example.json")))
    vae.update(model_path=str(tmp_path / "no_vae_run"))
    json.dump(vae, open(tmp_path / "vae.json", "w"))
    cfg = json.load(open(os.path.join(ROOT, "configs", "dalle_example.json")))
    cfg.update(n_layers=1, n_embd=128, n_heads=2, predict_batch_size=4, eval_batch_size=4, allow_random_vae=True,
               vae_model=str(tmp_path / "vae.json"), model_path=str(tmp_path / "no_run"), kv_cache_dtype="bf16")
    json.dump(cfg, open(tmp_path / "cfg.json", "w"))
    out = tmp_path / "out"
    args = ["--model", str(tmp_path / "cfg.json"), "--from-eval", "4", "--batch", "4", "--seed", "11", "--no-images", "--out", str(out),
            "--kv-cache-dtype", "fp8"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_dalle.py")] + args, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    info = json.load(open(out / "generate.json"))
    assert info["kv_cache_dtype"] == "fp8" and list(info)[-1] == "kv_cache_dtype"
    toks = np.load(out / "tokens.npy")
    assert toks.shape[0] == 4 and toks.min() >= 0 and np.isfinite(np.load(out / "logprob.npy")).all()
