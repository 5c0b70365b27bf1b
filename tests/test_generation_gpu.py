"""Generation on the MI355X: the nucleus draw (dmi_sample_tokens_p) against dmi_sample_tokens and the numpy restatement of its
kept set; image completion reproducing sampling bit for bit; the KV cache under recompute_grad; the model's log-likelihood of
its samples; and generate_dalle.py end to end."""
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
from nucleus_ref import nucleus_keep  # noqa: E402


def _rows(nv, B=5):
    g = torch.Generator().manual_seed(nv + 1)
    z = (torch.randn(B, nv + 8, generator=g) * 2).to(torch.bfloat16)
    z[1, 7] = z[1, 3] = z[1].float().max() + 1          # a tie of the maximum
    z[2, 20] = z[2, 10] = z[2].float().max() + 1
    z[3] = torch.round(z[3].float() / 2)                 # few distinct values: ties at tau (drawn without the bias below)
    bias = (torch.randn(nv, generator=g) * 0.5).to(torch.bfloat16)
    bias[7] = bias[3]
    bias[20] = bias[10]
    return z, bias, z[:, :nv].float() + bias.float()


def _scaled(v, T):
    return (v * torch.tensor(np.float32(1) / np.float32(T))).numpy().astype(np.float32)


@pytest.mark.parametrize("nv", [64, 512, 2048, 8192])
def test_nucleus_draw_kernel(nv):
    import dalle_hip as dh
    B = 5
    z, bias, v = _rows(nv, B)
    zd, bd = z.cuda(), bias.cuda()
    o1 = torch.zeros(B, 1, dtype=torch.int32, device="cuda")
    o2 = torch.zeros(B, 1, dtype=torch.int32, device="cuda")
    # top_p = 1: bit for bit dmi_sample_tokens, over (seed, position, temperature, top_k)
    rng = np.random.default_rng(nv)
    for it in range(60):
        T = [0.0, 0.5, 1.0, 1.7][it % 4]
        k = [0, 1, 6, nv // 3, nv][it % 5]
        seed, pos = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 20))
        dh.sample_tokens(zd, nv + 8, bd, B, nv, temperature=T, top_k=k, seed=seed, pos=pos, out=o1, out_col0=pos)
        dh.sample_tokens_p(zd, nv + 8, bd, B, nv, temperature=T, top_k=k, seed=seed, top_p=1.0, pos=pos, out=o2, out_col0=pos)
        assert torch.equal(o1, o2), (T, k, seed, pos)
    # greedy ignores top_p
    dh.sample_tokens_p(zd, nv + 8, bd, B, nv, temperature=0.0, top_p=0.01, pos=0, out=o2, out_col0=0)
    want = torch.stack([(v[b] == v[b].max()).nonzero()[0, 0] for b in range(B)]).to(torch.int32)
    assert torch.equal(o2[:, 0].cpu(), want)
    # no draw outside the restated nucleus set
    N = 1500
    for T, k, p in ((1.0, 0, 0.9), (0.7, 0, 0.5), (1.3, 40, 0.8), (1.0, 0, 1e-4)):
        draws = torch.zeros(B, N, dtype=torch.int32, device="cuda")
        for pos in range(N):
            dh.sample_tokens_p(zd, nv + 8, bd, B, nv, temperature=T, top_k=k, seed=11, top_p=p, pos=pos, out=draws, out_col0=0)
        draws = draws.cpu().numpy()
        for b in range(B):
            keep = nucleus_keep(_scaled(v[b], T), k, p)
            assert keep[draws[b]].all(), (T, k, p, b, int(keep.sum()))
            if p < 1e-3:
                vs = _scaled(v[b], T)
                assert keep.sum() == (vs == vs.max()).sum(), (b, int(keep.sum()))        # the maximum and its ties alone
    # ties at tau: a row of a few distinct values (no bias), every tied entry at the nucleus edge is drawn
    zt = z[3:4].cuda()
    vt = z[3, :nv].float()
    for T, p in ((1.0, 0.6), (0.5, 0.9)):
        draws = torch.zeros(1, N, dtype=torch.int32, device="cuda")
        for pos in range(N):
            dh.sample_tokens_p(zt, nv + 8, None, 1, nv, temperature=T, seed=3, top_p=p, pos=pos, out=draws, out_col0=0)
        keep = nucleus_keep(_scaled(vt, T), 0, p)
        d = draws[0].cpu().numpy()
        assert keep[d].all(), (T, p, int(keep.sum()))
    # distribution: 40 000 draws against the renormalised q over the kept set
    T, k, p = 0.8, 0, 0.9
    N = 40000
    draws = torch.zeros(B, N, dtype=torch.int32, device="cuda")
    for pos in range(N):
        dh.sample_tokens_p(zd, nv + 8, bd, B, nv, temperature=T, top_k=k, seed=9, top_p=p, pos=pos, out=draws, out_col0=0)
    draws = draws.cpu().long()
    for b in range(B):
        vb = torch.from_numpy(_scaled(v[b], T))
        keep = torch.from_numpy(nucleus_keep(vb.numpy(), k, p))
        prob = torch.softmax(vb.double().masked_fill(~keep, float("-inf")), -1)
        freq = torch.bincount(draws[b], minlength=nv).double() / N
        assert bool((freq[~keep] == 0).all()), b
        sigma = torch.sqrt(prob * (1 - prob) / N)
        assert bool(((freq - prob).abs() <= 5 * sigma + 1e-4).all()), (b, float((freq - prob).abs().max()))
    # by value == params_dev / pos_dev == advance
    seed = (123 << 32) | 77
    dh.sample_tokens_p(zd, nv + 8, bd, B, nv, temperature=T, top_k=6, seed=seed, top_p=0.7, pos=4, out=o1, out_col0=4)
    prm = dh.sample_params(T, 6, seed, top_p=0.7).cuda()
    dh.sample_tokens_p(zd, nv + 8, bd, B, nv, params_dev=prm, pos_dev=torch.tensor([4], dtype=torch.int32, device="cuda"),
                       out=o2, out_col0=4)
    assert torch.equal(o1, o2)
    pd = torch.tensor([0, 0], dtype=torch.int32, device="cuda")
    seq = torch.zeros(B, 6, dtype=torch.int32, device="cuda")
    for _ in range(6):
        dh.sample_tokens_p(zd, nv + 8, bd, B, nv, params_dev=dh.sample_params(T, k, 9, top_p=p).cuda(), pos_dev=pd, advance=True,
                           out=seq, out_col0=0)
    assert pd.cpu().tolist() == [6, 0] and torch.equal(seq.cpu().long(), draws[:, :6])
    # logp: log_softmax of (z + bias) in fp32 at the drawn index, accumulated over calls
    lsm = torch.log_softmax(v, -1)
    for T, k, p in ((1.0, 0, 1.0), (0.6, 5, 0.8), (0.0, 0, 1.0)):
        lp = torch.zeros(B, dtype=torch.float32, device="cuda")
        want = torch.zeros(B, dtype=torch.float64)
        for pos in range(3):
            dh.sample_tokens_p(zd, nv + 8, bd, B, nv, temperature=T, top_k=k, seed=5, top_p=p, pos=pos, out=o1, out_col0=pos,
                               logp=lp)
            want += lsm[torch.arange(B), o1[:, 0].cpu().long()].double()
        got = lp.cpu().double()
        assert bool(((got - want).abs() <= 2e-5 * (1 + want.abs())).all()), (T, k, p, got, want)


# ---------------------------------------------------------------- the engine
def _engine(d, H, seed=9, **hp):
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    T, P, tv, iv, B = 16, 48, 60, 64, 3
    cfg = do.DalleConfig(d, tv, iv, T, P, 2, H)
    eng = DalleEngine(d, 2, H, tv, iv, T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10, **hp))
    eng.load_reference_params(do.init_params(cfg, seed=seed, perturb=0.05))
    text = torch.from_numpy(do.synthetic_captions(B, T, tv, seed=1)).cuda()
    return eng, text


def _near_tie_rule(eng, text, a, b, tol):
    """a (cached) and b (plain) greedy samples agree up to the first disagreement, which must be a near-tie of the full
    forward's logits (test_kv_cached_decode_equals_full_forward)"""
    B, T, S, P, tv, iv = eng.B, eng.T, eng.S, eng.S - eng.T, eng.text_vocab_size, eng.image_vocab_size
    for i in range(B):
        bad = (a[i] != b[i]).nonzero()
        if len(bad) == 0:
            continue
        f = int(bad[0])
        seq = torch.cat([text[i].to(torch.int32), b[i, :f].to(torch.int32) + tv,
                         torch.full((P - f,), tv, dtype=torch.int32, device="cuda")])
        eng.forward(seq.repeat(B, 1), need_grad=False)
        zz = eng.z.view(B, S, eng.Vp)[0, T + f - 1, tv:tv + iv].float()
        top2 = zz.topk(2).values
        assert float(top2[0] - top2[1]) <= tol, (i, f, float(top2[0] - top2[1]))


MODES = {"greedy": dict(temperature=0.0), "top_k": dict(temperature=1.0, top_k=8, seed=3),
         "top_p": dict(temperature=1.0, top_p=0.9, seed=5)}


@pytest.mark.parametrize("d,H", [(128, 1), (128, 2)])      # head dims 128 and 64
def test_completion_reproduces_sampling_exactly(d, H):
    from src.dalle_mtf.engine import Draw
    eng, text = _engine(d, H)
    P = eng.S - eng.T
    for name, kw in MODES.items():
        s = eng.sample_image_tokens(text, **kw)
        assert int(s.min()) >= 0 and int(s.max()) < eng.image_vocab_size
        for path in (dict(), dict(fused_sampling=False)):
            assert torch.equal(eng.sample_image_tokens(text, **kw, **path), s), (name, path)
            for k in (1, 17, P - 1):
                c = eng.sample_image_tokens(text, image_prefix=s[:, :k], **kw, **path)
                assert torch.equal(c, s), (name, path, k, (c != s).nonzero()[:3])
        if name == "greedy":
            plain = eng.sample_image_tokens(text, kv_cache=False, **kw)
            _near_tie_rule(eng, text, s, plain, 0.05)
            cp = eng.sample_image_tokens(text, kv_cache=False, image_prefix=s[:, :17], **kw)
            assert torch.equal(cp[:, :17], s[:, :17])
    assert all(k in eng._dec["graphs"] for k in (Draw(True, False, False), Draw(False, False, False), False))
    with pytest.raises(ValueError):
        eng.sample_image_tokens(text, image_prefix=torch.zeros(3, P, dtype=torch.int32))
    with pytest.raises(ValueError):
        eng.sample_image_tokens(text, image_prefix=torch.full((3, 2), eng.image_vocab_size, dtype=torch.int32))
    with pytest.raises(ValueError):
        eng.sample_image_tokens(text, top_p=0.0)


def test_every_draw_variant_is_bit_identical_across_the_decode_paths():
    """the fused graph, the host-launched draw and the eager decode step launch the same draw kernel on the same bits: the same
    tokens and the same logp, exactly, for the plain, the nucleus + logp and the guided variant (B = 2: one pair)"""
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine, Draw
    T, P, tv, iv, B = 16, 48, 60, 64, 2
    eng = DalleEngine(128, 1, 1, tv, iv, T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10))
    eng.load_reference_params(do.init_params(do.DalleConfig(128, tv, iv, T, P, 1, 1), seed=9, perturb=0.05))
    text = torch.from_numpy(do.synthetic_captions(B, T, tv, seed=1)).cuda()
    seed = (5 << 32) | 11
    variants = ((Draw(False, False, False), text, dict(temperature=1.0, top_k=8, seed=seed)),
                (Draw(True, False, True), text, dict(temperature=0.9, top_k=12, top_p=0.8, seed=seed, return_logprobs=True)),
                (Draw(True, True, True), text[:1], dict(temperature=1.0, top_p=0.9, seed=seed, guidance_scale=2.0, return_logprobs=True)))
    for key, txt, kw in variants:
        fused = eng.sample_image_tokens(txt, **kw)
        assert key in eng._dec["graphs"], key
        for path in (dict(fused_sampling=False), dict(decode_graph=False)):
            got = eng.sample_image_tokens(txt, **kw, **path)
            if key.logp:
                assert fused[0].shape == (len(txt), P) and torch.equal(got[0], fused[0]), (key, path)
                assert torch.equal(got[1], fused[1]), (key, path, got[1], fused[1])
            else:
                assert fused.shape == (len(txt), P) and torch.equal(got, fused), (key, path)
    assert set(eng._dec["graphs"]) == {False} | {key for key, _, _ in variants}     # one graph per variant


def test_recompute_engine_samples_from_its_own_kv_cache():
    eng, text = _engine(128, 1, recompute_grad=True)
    ref, _ = _engine(128, 1)
    assert eng.recompute and not ref.recompute
    calls = []
    fwd = eng.forward

    def counting(*a, **k):
        calls.append(1)
        return fwd(*a, **k)
    eng.forward = counting
    a = eng.sample_image_tokens(text, temperature=0.0)
    assert len(calls) == 1, len(calls)
    kv = [t.data_ptr() for t in eng._kv]
    assert len(set(kv)) == eng.L and eng._kv[0].shape == (eng.B * eng.S, 3 * eng.d)
    a2 = eng.sample_image_tokens(text, temperature=0.0)
    a3 = eng.sample_image_tokens(text, temperature=1.0, top_p=0.8, seed=2, return_logprobs=True)[0]
    torch.cuda.synchronize()
    assert len(calls) == 3 and [t.data_ptr() for t in eng._kv] == kv
    mem = torch.cuda.memory_allocated()
    a4 = eng.sample_image_tokens(text, temperature=0.0)
    eng.sample_image_tokens(text, temperature=1.0, top_p=0.8, seed=2, return_logprobs=True)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() <= mem + (1 << 20), (torch.cuda.memory_allocated(), mem)
    assert [t.data_ptr() for t in eng._kv] == kv
    assert torch.equal(a, a2) and torch.equal(a, a4) and int(a3.max()) < eng.image_vocab_size
    eng.forward = fwd
    b = ref.sample_image_tokens(text, temperature=0.0)
    _near_tie_rule(ref, text, a, b, 0.05)
    plain = eng.sample_image_tokens(text, temperature=0.0, kv_cache=False)
    _near_tie_rule(eng, text, a, plain, 0.05)
    # the training step still runs on its shared buffers
    loss = eng.train_step(torch.cat([text, a + eng.text_vocab_size], 1).to(torch.int32))
    assert bool(torch.isfinite(loss).all())


def test_return_logprobs_is_the_sum_of_decode_step_log_softmax():
    eng, text = _engine(128, 1)
    B, T, S = eng.B, eng.T, eng.S
    tv = eng.text_vocab_size
    for kw in (dict(temperature=1.0, top_p=0.9, seed=7), dict(temperature=0.8, top_k=5, seed=1), dict(temperature=0.0)):
        for path in (dict(), dict(fused_sampling=False)):
            toks, lp = eng.sample_image_tokens(text, return_logprobs=True, **kw, **path)
            assert lp.shape == (B,) and lp.dtype == torch.float32
            plain_toks = eng.sample_image_tokens(text, **kw, **path)
            if kw.get("top_p", 1.0) == 1.0:
                assert torch.equal(plain_toks, toks)    # the nucleus kernel at top_p = 1 draws what the top-k kernel draws
            full = torch.cat([text.to(torch.int32), toks.to(torch.int32) + tv], 1)
            eng._prefill(full)
            want = torch.zeros(B, dtype=torch.float64)
            for pos in range(T - 1, S - 1):
                z = eng.decode_step(full[:, pos].contiguous(), pos).double().cpu()
                want += torch.log_softmax(z, -1)[torch.arange(B), toks[:, pos - T + 1].cpu().long()]
            got = lp.double().cpu()
            assert bool(((got - want).abs() <= 1e-4 * want.abs()).all()), (kw, path, got, want)
    # a prefix adds nothing: the score of a completion sums the drawn positions only
    s, lp = eng.sample_image_tokens(text, temperature=1.0, top_p=0.9, seed=7, return_logprobs=True)
    c, lpc = eng.sample_image_tokens(text, temperature=1.0, top_p=0.9, seed=7, return_logprobs=True, image_prefix=s[:, :10])
    assert torch.equal(c, s) and bool((lpc > lp).all())


# ---------------------------------------------------------------- the CLI
def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "generate_dalle.py")] + args, cwd=cwd, env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def test_generate_cli_end_to_end(tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "configs", "dalle_example.json")))
    cfg.update(n_layers=1, n_embd=256, n_heads=2, predict_batch_size=4, allow_random_vae=True,
               model_path=str(tmp_path / "no_run"))
    vae = json.load(open(os.path.join(ROOT, "configs", "vae_example.json")))
    vae.update(model_path=str(tmp_path / "no_vae_run"))
    json.dump(vae, open(tmp_path / "vae.json", "w"))
    cfg["vae_model"] = str(tmp_path / "vae.json")
    json.dump(cfg, open(tmp_path / "tiny.json", "w"))
    base = ["--model", str(tmp_path / "tiny.json"), "--from-eval", "6", "--samples-per-caption", "2", "--batch", "4", "--top-p", "0.9"]
    _cli(base + ["--out", str(tmp_path / "a")], str(tmp_path))
    _cli(base + ["--out", str(tmp_path / "b")], str(tmp_path))
    a = tmp_path / "a"
    toks = np.load(a / "tokens.npy")
    caps = np.load(a / "captions.npy")
    lp = np.load(a / "logprob.npy")
    assert toks.shape == (12, 16) and toks.dtype == np.int32 and toks.min() >= 0 and toks.max() < 512
    assert caps.shape == (6, 256) and lp.shape == (12,) and lp.dtype == np.float32
    assert np.isfinite(lp).all() and (lp < 0).all() and (lp > 16 * np.log(1.0 / 512) - 50).all()
    pngs = sorted(f for f in os.listdir(a) if f.endswith(".png"))
    assert len(pngs) == 12 and "0_0.png" in pngs and "5_1.png" in pngs
    from PIL import Image
    im = np.asarray(Image.open(a / "3_1.png"))
    assert im.shape == (32, 32, 3) and im.dtype == np.uint8
    info = json.load(open(a / "generate.json"))
    assert info["top_p"] == 0.9 and info["rows"] == 12 and info["batches"] == 3 and info["seconds"]["sample"] > 0
    assert np.array_equal(toks, np.load(tmp_path / "b" / "tokens.npy"))
    assert not all(np.array_equal(toks[2 * i], toks[2 * i + 1]) for i in range(6))    # the samples of a caption differ
    # completion of the eval images from their first K tokens
    _cli(base + ["--image-prefix", "5", "--out", str(tmp_path / "c")], str(tmp_path))
    c = np.load(tmp_path / "c" / "tokens.npy")
    assert c.shape == (12, 16) and np.array_equal(np.load(tmp_path / "c" / "captions.npy"), caps)
    # the eval images' tokens, as the training step tokenises them
    import dalle_hip as dh
    from src.input_fns import dalle_input_fn
    from src.model_fns import initialize_vae_weights, load_vae_model
    from src.utils import fetch_model_params
    params = fetch_model_params(str(tmp_path / "tiny.json"))
    params["vae_params"] = fetch_model_params(str(tmp_path / "vae.json"))
    params.update(padding_id=50257, batch_size=4, _tokenizer_batch=4)
    v, ck = load_vae_model(params, "predict")
    initialize_vae_weights(v, ck)
    imgs = []
    it = dalle_input_fn(params, eval=True)
    while sum(len(x) for x in imgs) < 6:
        imgs.append(next(it)[0].numpy())
    imgs = np.concatenate(imgs)[:8]
    want = np.empty((8, 16), np.int32)
    buf = torch.empty(4, 256 + 16, dtype=torch.int32, device="cuda")
    for c0 in (0, 4):
        logits = v.forward(torch.from_numpy(imgs[c0:c0 + 4]).cuda(), return_logits=True)
        dh.assemble_tokens(torch.zeros(4, 256, dtype=torch.int32, device="cuda"), logits.contiguous(), buf, 4, 256, 16,
                           logits.shape[-1], 0)
        want[c0:c0 + 4] = buf[:, 256:].cpu().numpy()
    assert np.array_equal(c[:, :5], np.repeat(want[:6, :5], 2, 0))
