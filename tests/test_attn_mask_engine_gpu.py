"""Custom attention masks through the engine and DALLE on the GPU: the train step against a masked fp32 oracle, causal vs
absent config key, recompute_grad, decode against the full forward, and the samplers."""
import pytest
import torch

from engine_case import IV, P, PATTERNS, T, TV, build, step
from parity import rel_l2

pytestmark = pytest.mark.gpu


def _setup(patterns=PATTERNS, **hp):
    return build(hparams=dict(hp, attention_pattern=patterns))


def test_engine_step_with_per_layer_masks_vs_masked_fp32_oracle():
    import dalle_step_ref as sref
    from src.dalle_mtf.masks import layer_masks
    cfg, model, P0, tokens = _setup()
    eng = model.engine
    assert all(p is not None for p in eng.attn_plan)
    loss = float(step(eng, tokens)[0].item())
    gh = eng.export_reference(eng.g)
    loss_o, go = sref.loss_and_grads(P0, tokens, cfg, masks=layer_masks(PATTERNS, cfg.n_layers, T, P))
    assert abs(loss - loss_o) <= 5e-4 * abs(loss_o), (loss, loss_o)
    worst = max((rel_l2(gh[k], go[k]), k) for k in go)
    print("masked engine vs masked fp32 oracle: loss", loss, loss_o, "worst grad", worst, flush=True)
    assert worst[0] <= 4.8e-2, worst   # the causal step's bound (tests/parity.py check_report)
    # the masks matter: the causal oracle is far from the engine
    import oracle.dalle_oracle as do
    loss_c, gc = do.loss_and_grads(P0, tokens, cfg)
    assert max(rel_l2(gh[k], gc[k]) for k in gc) > 0.2


def test_causal_pattern_and_absent_key_are_bit_identical():
    out = []
    for patterns in ("causal", "absent", ["causal"] * 3):
        _, model, _, tokens = _setup(patterns)
        eng = model.engine
        assert all(p is None for p in eng.attn_plan)
        out.append(step(eng, tokens))
        del model, eng
        torch.cuda.empty_cache()
    for loss, g in out[1:]:
        assert torch.equal(loss, out[0][0]) and torch.equal(g, out[0][1])


def test_recompute_grad_with_masks_equals_stored_activations():
    res = []
    for rc in (False, True):
        _, model, _, tokens = _setup(recompute_grad=rc)
        res.append(step(model.engine, tokens))
        del model
        torch.cuda.empty_cache()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_masked_decode_logits_and_samplers():
    """decode logits equal full-forward logits at every image position (the decode tolerance of test_model_fns_gpu.py); the
    graph-replayed and host-launched samplers give the same tokens; greedy cached tokens equal the plain sampler's up to near-ties"""
    _, model, _, tokens = _setup()
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
