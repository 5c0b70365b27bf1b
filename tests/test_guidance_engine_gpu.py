"""Classifier-free guidance on the MI355X through the engine: DalleEngine.sample_image_tokens(guidance_scale=, uncond_text=)
against a host restatement built from decode_step's logits, against the unguided sampler where the two must coincide, across
its decode paths, with image completion and logp, its refusals, and generate_dalle.py --guidance-scale end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guidance_ref import guided_logits  # noqa: E402

T, P, TV, IV, B = 16, 48, 60, 64, 4
BC = B // 2
SHAPES = [(256, 2), (128, 2)]         # head dims 128 and 64
_ENGINES = {}


def _engine(d, H):
    """the shapes of test_generation_gpu._engine at an even batch; one engine per shape for the whole module"""
    if (d, H) not in _ENGINES:
        from oracle import dalle_oracle as do
        from src.dalle_mtf.engine import DalleEngine
        cfg = do.DalleConfig(d, TV, IV, T, P, 2, H)
        eng = DalleEngine(d, 2, H, TV, IV, T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10))
        eng.load_reference_params(do.init_params(cfg, seed=9, perturb=0.05))
        text = torch.from_numpy(do.synthetic_captions(B, T, TV, seed=1)).cuda()
        _ENGINES[(d, H)] = (eng, text)
    return _ENGINES[(d, H)]


def _draw(nucleus=False, guided=False, logp=False):
    """the engine's key of a draw variant's captured graph"""
    from src.dalle_mtf.engine import Draw
    return Draw(nucleus, guided, logp)


def _null(n=None):
    t = torch.full((T,), TV - 1, dtype=torch.int32, device="cuda")     # no padding_id in the hparams: text_vocab_size - 1
    return t if n is None else t.repeat(n, 1)


@pytest.mark.parametrize("d,H", SHAPES)
def test_scale_one_without_uncond_text_is_the_unguided_sampler(d, H):
    eng, text = _engine(d, H)
    before = set((getattr(eng, "_dec", None) or {}).get("graphs", {}))
    for kw in (dict(temperature=0.0), dict(temperature=1.0, top_k=8, seed=3), dict(temperature=1.0, top_p=0.9, seed=5)):
        a = eng.sample_image_tokens(text, **kw)
        b = eng.sample_image_tokens(text, guidance_scale=1.0, uncond_text=None, **kw)
        assert a.shape == (B, P) and torch.equal(a, b), kw
    assert set(eng._dec["graphs"]) - before <= {_draw(), _draw(nucleus=True)}             # the unguided graphs, no guided one


@pytest.mark.parametrize("d,H", SHAPES)
def test_guided_greedy_equals_the_host_combination_of_decode_step_logits(d, H):
    eng, text = _engine(d, H)
    cap = text[:BC]
    for scale in (3.0, 0.5):
        toks = torch.full((B, T + P), TV, dtype=torch.int32, device="cuda")
        toks[:BC, :T] = cap
        toks[BC:, :T] = _null(BC)
        eng.forward(toks, need_grad=False)                      # the prefill: k, v of the text positions
        want = np.zeros((BC, P), np.int64)
        cur = toks[:, T - 1].contiguous()
        for i in range(P):
            lg = eng.decode_step(cur, T - 1 + i).cpu().numpy()
            c = np.argmax(guided_logits(lg[:BC], lg[BC:], scale), -1)           # first maximum
            want[:, i] = c
            cur = torch.from_numpy(np.concatenate([c, c]).astype(np.int32) + TV).cuda()
        got = eng.sample_image_tokens(cap, temperature=0.0, guidance_scale=scale)
        assert got.shape == (BC, P) and got.dtype == torch.int32
        assert np.array_equal(got.cpu().numpy(), want), (scale, (got.cpu().numpy() != want).nonzero())
        # the default unconditional caption is the null caption, as one row or as one per pair
        assert torch.equal(eng.sample_image_tokens(cap, temperature=0.0, guidance_scale=scale, uncond_text=_null()), got)
        assert torch.equal(eng.sample_image_tokens(cap, temperature=0.0, guidance_scale=scale, uncond_text=_null(BC).cpu().long()), got)
    assert not torch.equal(eng.sample_image_tokens(cap, temperature=0.0, guidance_scale=3.0),
                           eng.sample_image_tokens(cap, temperature=0.0, guidance_scale=0.5))


@pytest.mark.parametrize("d,H", SHAPES)
def test_equal_halves_draw_the_unguided_tokens_of_their_pair(d, H):
    """uncond_text == text: g == zc at any scale, so pair b draws what row b of an unguided batch [captions; captions] draws
    (same noise: the pair index is the row index) -- a wrong pairing or a draw fed to one half only would show here"""
    eng, text = _engine(d, H)
    cap = text[:BC]
    dup = torch.cat([cap, cap])
    toks = torch.full((B, T + P), TV, dtype=torch.int32, device="cuda")
    toks[:, :T] = dup
    eng.forward(toks, need_grad=False)
    cur = toks[:, T - 1].contiguous()
    for i in range(4):                                           # the two halves' logits are bit-equal (row-independent decode)
        lg = eng.decode_step(cur, T - 1 + i)
        assert torch.equal(lg[:BC], lg[BC:]), i
        cur = (lg.argmax(-1).to(torch.int32) + TV).contiguous()
    for kw in (dict(temperature=0.0), dict(temperature=1.0, top_k=8, seed=3), dict(temperature=0.9, top_p=0.9, seed=5)):
        plain = eng.sample_image_tokens(dup, **kw)
        got = eng.sample_image_tokens(cap, guidance_scale=3.0, uncond_text=cap, **kw)
        assert torch.equal(got, plain[:BC]), kw
        got1 = eng.sample_image_tokens(cap, guidance_scale=1.0, uncond_text=_null(), **kw)   # scale 1: the uncond rows do not matter
        assert torch.equal(got1, plain[:BC]), kw


@pytest.mark.parametrize("d,H", SHAPES)
def test_guided_decode_paths_completion_and_logp(d, H):
    eng, text = _engine(d, H)
    cap = text[:BC]
    for kw in (dict(temperature=1.0, top_k=8, seed=3), dict(temperature=1.0, top_p=0.9, seed=5), dict(temperature=0.0)):
        kw = dict(kw, guidance_scale=2.5)
        s = eng.sample_image_tokens(cap, **kw)
        assert s.shape == (BC, P) and int(s.min()) >= 0 and int(s.max()) < IV
        for path in (dict(fused_sampling=False), dict(decode_graph=False)):
            assert torch.equal(eng.sample_image_tokens(cap, **kw, **path), s), (kw, path)
        for k in (1, 17, P - 1):                                 # sampling s, then completing s[:, :k], returns s
            for path in (dict(), dict(fused_sampling=False)):
                c = eng.sample_image_tokens(cap, image_prefix=s[:, :k], **kw, **path)
                assert torch.equal(c, s), (kw, path, k)
        toks, lp = eng.sample_image_tokens(cap, return_logprobs=True, **kw)
        toks2, lp2 = eng.sample_image_tokens(cap, return_logprobs=True, fused_sampling=False, **kw)
        assert torch.equal(toks, s) and torch.equal(toks2, s)
        assert lp.shape == (BC,) and lp.dtype == torch.float32 and torch.equal(lp, lp2)
        # logp is the conditional rows' own score: the sum of log_softmax of their decode_step logits at the drawn tokens
        full = torch.full((B, T + P), TV, dtype=torch.int32, device="cuda")
        full[:BC, :T] = cap
        full[BC:, :T] = _null(BC)
        full[:, T:] = torch.cat([s, s]) + TV
        eng.forward(full, need_grad=False)
        want = torch.zeros(BC, dtype=torch.float64)
        for pos in range(T - 1, T + P - 1):
            z = eng.decode_step(full[:, pos].contiguous(), pos).double().cpu()
            want += torch.log_softmax(z[:BC], -1)[torch.arange(BC), s[:, pos - T + 1].cpu().long()]
        got = lp.double().cpu()
        assert bool(((got - want).abs() <= 1e-4 * want.abs()).all()), (kw, got, want)
    assert _draw(True, True) in eng._dec["graphs"] and _draw(True, True, True) in eng._dec["graphs"]
    # the plain sampler (one full forward per position) by the agreement rule of the masked engine test
    g = eng.sample_image_tokens(cap, temperature=0.0, guidance_scale=2.5)
    b = eng.sample_image_tokens(cap, temperature=0.0, guidance_scale=2.5, kv_cache=False)
    assert b.shape == (BC, P)
    agree = float((g == b).float().mean())
    print("guided: cached vs uncached greedy tokens agree on", agree, flush=True)
    assert int((g != b).any(1).sum()) == 0 or agree >= 0.5, agree


def test_guidance_refusals():
    eng, text = _engine(256, 2)
    cap = text[:BC]
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="guidance_scale"):
            eng.sample_image_tokens(cap, guidance_scale=bad)
    with pytest.raises(ValueError, match="text must be"):
        eng.sample_image_tokens(text, guidance_scale=2.0)                      # B rows of text where B / 2 are wanted
    for bad in (torch.zeros(T + 1, dtype=torch.int32), torch.zeros(B, T, dtype=torch.int32), torch.zeros(BC, T, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="uncond_text must be"):
            eng.sample_image_tokens(cap, guidance_scale=2.0, uncond_text=bad)
    with pytest.raises(ValueError, match="integer"):
        eng.sample_image_tokens(cap, uncond_text=torch.zeros(T))
    for bad in (TV, -1):
        with pytest.raises(ValueError, match="uncond_text ids"):
            eng.sample_image_tokens(cap, uncond_text=torch.full((T,), bad, dtype=torch.int32))
    with pytest.raises(ValueError, match="image_prefix"):
        eng.sample_image_tokens(cap, guidance_scale=2.0, image_prefix=torch.zeros(B, 3, dtype=torch.int32))
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    odd = DalleEngine(128, 1, 1, TV, IV, T, P, batch_size=3, hparams=dict(lr=1e-3, train_steps=10))
    odd.load_reference_params(do.init_params(do.DalleConfig(128, TV, IV, T, P, 1, 1), seed=2, perturb=0.05))
    with pytest.raises(ValueError, match="even"):
        odd.sample_image_tokens(text[:1], guidance_scale=2.0)


def test_dalle_sample_passes_guidance_through():
    from src.dalle_mtf.models import DALLE
    m = DALLE(n_embd=256, text_vocab_size=TV, image_vocab_size=IV, text_seq_len=T, image_seq_len=P, n_layers=1, n_heads=2,
              batch_size=B, mode="predict", params=dict(padding_id=TV - 2))
    m.engine.init_params(seed=1)
    _, text = _engine(256, 2)
    cap = text[:BC]
    a = m.sample(cap, temperature=0.0, guidance_scale=2.0)
    assert a.shape == (BC, P)
    # the null caption follows the config's padding_id
    assert torch.equal(a, m.sample(cap, temperature=0.0, guidance_scale=2.0, uncond_text=torch.full((T,), TV - 2, dtype=torch.int32)))
    toks, lp = m.sample(cap, temperature=1.0, top_p=0.9, seed=1, guidance_scale=2.0, return_logprobs=True)
    assert toks.shape == (BC, P) and lp.shape == (BC,)


def test_no_garbage_is_finalised_inside_a_decode_graph_capture():
    """cyclic garbage that is dead when a sampler captures its graph is finalised before the capture, the collector is off while
    the stream captures and back on afterwards: a finaliser inside a capture (a dead model's CUDAGraph synchronises the device
    when it is destroyed) is an illegal call there and aborts the process"""
    import gc
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    eng = DalleEngine(128, 1, 1, TV, IV, T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10))
    eng.load_reference_params(do.init_params(do.DalleConfig(128, TV, IV, T, P, 1, 1), seed=4, perturb=0.05))
    _, text = _engine(256, 2)
    seen = []

    class Node:
        def __del__(self):
            seen.append(bool(torch.cuda.is_current_stream_capturing()))

    body = eng._decode_body
    inside = []

    def watched(sample=False):
        if torch.cuda.is_current_stream_capturing():
            inside.append(gc.isenabled())
            a, b = Node(), Node()
            a.other, b.other = b, a                  # garbage born inside the capture stays until it is over
        return body(sample)
    eng._decode_body = watched
    assert gc.isenabled()
    gc.collect()
    gc.disable()                                     # so that the cycle below is still there when the sampler captures
    try:
        a, b = Node(), Node()
        a.other, b.other = b, a
        del a, b
        assert seen == []
        toks = eng.sample_image_tokens(text[:BC], temperature=0.0, guidance_scale=2.0)
        assert _draw(True, True) in eng._dec["graphs"] and inside == [False]
        assert seen[:2] == [False, False], seen      # finalised by the collection in front of the capture, not inside it
        assert not gc.isenabled()                    # the collector is left as it was found
    finally:
        gc.enable()
    assert torch.equal(eng.sample_image_tokens(text[:BC], temperature=0.0, guidance_scale=2.0), toks)
    gc.collect()
    assert len(seen) == 4 and not any(seen), seen
    assert gc.isenabled() and _draw() not in eng._dec["graphs"]
    eng.sample_image_tokens(text, temperature=0.0)   # one more capture, with the collector on: it is on again afterwards
    assert _draw() in eng._dec["graphs"] and gc.isenabled() and inside == [False, False]
    eng._decode_body = body


# ---------------------------------------------------------------- the CLI
def test_generate_cli_with_guidance(tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "configs", "dalle_example.json")))
    cfg.update(n_layers=1, n_embd=256, n_heads=2, predict_batch_size=4, allow_random_vae=True, model_path=str(tmp_path / "no_run"))
    vae = json.load(open(os.path.join(ROOT, "configs", "vae_example.json")))
    vae.update(model_path=str(tmp_path / "no_vae_run"))
    json.dump(vae, open(tmp_path / "vae.json", "w"))
    cfg["vae_model"] = str(tmp_path / "vae.json")
    json.dump(cfg, open(tmp_path / "tiny.json", "w"))
    args = ["--model", str(tmp_path / "tiny.json"), "--from-eval", "6", "--samples-per-caption", "2", "--batch", "4", "--top-p", "0.9",
            "--guidance-scale", "2", "--out", str(tmp_path / "g")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_dalle.py")] + args, cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    g = tmp_path / "g"
    toks, caps, lp = np.load(g / "tokens.npy"), np.load(g / "captions.npy"), np.load(g / "logprob.npy")
    assert toks.shape == (12, 16) and toks.dtype == np.int32 and toks.min() >= 0 and toks.max() < 512
    assert caps.shape == (6, 256) and lp.shape == (12,) and np.isfinite(lp).all() and (lp < 0).all()
    pngs = sorted(f for f in os.listdir(g) if f.endswith(".png"))
    assert len(pngs) == 12 and "0_0.png" in pngs and "5_1.png" in pngs
    info = json.load(open(g / "generate.json"))
    assert info["guidance_scale"] == 2.0 and info["rows"] == 12 and info["batch"] == 4 and info["batches"] == 6
