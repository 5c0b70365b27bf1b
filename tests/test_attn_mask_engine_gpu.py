"""Custom attention masks through the engine and DALLE on the GPU: the train step against a masked fp32 oracle, causal vs
absent config key, recompute_grad, decode against the full forward, and the samplers."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T, P, TV, IV = 16, 256, 300, 64
PATTERNS = ["row", "column", "conv:3"]


def _setup(n_embd=256, n_heads=2, n_layers=3, B=2, seed=0, patterns=PATTERNS, hp=None):
    from oracle import dalle_oracle as do
    from src.dalle_mtf.models import DALLE
    cfg = do.DalleConfig(n_embd, TV, IV, T, P, n_layers, n_heads)
    params = dict(hp or dict(lr=1e-3, train_steps=1000, warmup_steps=2, gradient_clipping=1.0))
    if patterns is not None:
        params["attention_pattern"] = patterns
    model = DALLE(n_embd=n_embd, text_vocab_size=TV, image_vocab_size=IV, text_seq_len=T, image_seq_len=P, n_layers=n_layers,
                  n_heads=n_heads, batch_size=B, params=params)
    P0 = do.init_params(cfg, seed=1234 + seed, perturb=0.05)
    model.engine.load_reference_params(P0)
    tokens = do.assemble_tokens(do.synthetic_captions(B, T, TV, seed=seed + 1), do.synthetic_image_tokens(B, P, IV, seed=seed + 2), TV)
    return cfg, model, P0, tokens


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-30))


def test_engine_step_with_per_layer_masks_vs_masked_fp32_oracle():
    import masked_attention_ref as mref
    from src.dalle_mtf.masks import layer_masks
    cfg, model, P0, tokens = _setup()
    eng = model.engine
    assert all(p is not None for p in eng.attn_plan)
    loss = float(eng.forward(torch.from_numpy(tokens).cuda(), need_grad=True).item())
    eng.backward(allreduce=False)
    torch.cuda.synchronize()
    gh = eng.export_reference(eng.g)
    masks = layer_masks(PATTERNS, cfg.n_layers, T, P)
    loss_o, _, go = mref.loss_and_grads(P0, tokens, cfg, masks)
    assert abs(loss - loss_o) <= 5e-4 * abs(loss_o), (loss, loss_o)
    worst = max((_rel_l2(gh[k], go[k]), k) for k in go)
    print("masked engine vs masked fp32 oracle: loss", loss, loss_o, "worst grad", worst, flush=True)
    assert worst[0] <= 4.8e-2, worst   # the causal step's bound (tests/parity.py check_report)
    # the masks matter: the causal oracle is far from the engine
    import oracle.dalle_oracle as do
    loss_c, gc = do.loss_and_grads(P0, tokens, cfg)
    assert max(_rel_l2(gh[k], gc[k]) for k in gc) > 0.2


def test_causal_pattern_and_absent_key_are_bit_identical():
    out = []
    for patterns in ("causal", None, ["causal"] * 3):
        _, model, _, tokens = _setup(patterns=patterns)
        eng = model.engine
        assert all(p is None for p in eng.attn_plan)
        loss = eng.forward(torch.from_numpy(tokens).cuda(), need_grad=True).clone()
        eng.backward(allreduce=False)
        torch.cuda.synchronize()
        out.append((loss, eng.g.clone()))
        del model, eng
        torch.cuda.empty_cache()
    for loss, g in out[1:]:
        assert torch.equal(loss, out[0][0]) and torch.equal(g, out[0][1])


def test_recompute_grad_with_masks_equals_stored_activations():
    res = []
    for rc in (False, True):
        _, model, _, tokens = _setup(hp=dict(lr=1e-3, train_steps=1000, warmup_steps=2, gradient_clipping=1.0, recompute_grad=rc))
        eng = model.engine
        loss = eng.forward(torch.from_numpy(tokens).cuda(), need_grad=True).clone()
        eng.backward(allreduce=False)
        torch.cuda.synchronize()
        res.append((loss, eng.g.clone()))
        del model, eng
        torch.cuda.empty_cache()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_masked_decode_logits_and_samplers():
    """decode logits equal full-forward logits at every image position (the decode tolerance of test_model_fns_gpu.py); the
    graph-replayed and host-launched samplers give the same tokens; greedy cached tokens equal the plain sampler's up to near-ties"""
    _, model, _, tokens = _setup(n_embd=256, n_heads=2)
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    eng.forward(tok, need_grad=False)
    full = eng.logits()[:, :, TV:TV + IV].clone()
    eng._prefill(tok)
    worst = 0.0
    for pos in range(T - 1, T + P - 1):
        z = eng.decode_step(tok[:, pos].contiguous(), pos, graph=True).float()
        ref = full[:, pos]
        worst = max(worst, float((z - ref).abs().max() / ref.abs().max()))
    print("masked decode vs full forward logits: worst relative", worst, flush=True)
    assert worst <= 3e-2, worst
    text = tok[:, :T].contiguous()
    a = eng.sample_image_tokens(text, temperature=1.0, top_k=8, seed=3, kv_cache=True)
    a2 = eng.sample_image_tokens(text, temperature=1.0, top_k=8, seed=3, kv_cache=True, fused_sampling=False)
    a3 = eng.sample_image_tokens(text, temperature=1.0, top_k=8, seed=3, kv_cache=True, decode_graph=False)
    assert torch.equal(a, a2) and torch.equal(a, a3)
    g = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True)
    b = eng.sample_image_tokens(text, temperature=0.0, kv_cache=False)
    agree = float((g == b).float().mean())
    print("masked: cached vs uncached greedy tokens agree on", agree, flush=True)
    assert int((g != b).any(1).sum()) == 0 or agree >= 0.5, agree


def test_head_dim64_with_a_mask_is_refused():
    import dalle_hip as dh
    from src.dalle_mtf.models import DALLE
    with pytest.raises(dh.DalleHipError, match="head dim 128"):
        DALLE(n_embd=128, text_vocab_size=TV, image_vocab_size=IV, text_seq_len=T, image_seq_len=P, n_layers=2, n_heads=2,
              batch_size=1, attn_mask="row")
    DALLE(n_embd=128, text_vocab_size=TV, image_vocab_size=IV, text_seq_len=T, image_seq_len=P, n_layers=2, n_heads=2,
          batch_size=1, attn_mask="causal")
