"""Embedding / residual dropout on the GPU: the four dropout entry points bit for bit against the numpy restatement of the mask
(tests/dropout_ref.py), the engine's train step against the fp32 oracle with the same masks injected (tests/dalle_step_ref.py), and what the engine promises
around it: keys off = the parent's bits, recompute_grad, microbatches, steps, evaluation / sampling untouched, resume."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dalle_hip as dh  # noqa: E402  (path set up by conftest)
import dropout_ref as dref  # noqa: E402
from engine_case import BATCH, NL, P, T, build, step  # noqa: E402
from parity import rel_l2  # noqa: E402
from test_dropout import RATE, WIDTHS  # noqa: E402

DEV = "cuda"
KEY = 0x0123456789ABCDEF
SHAPES = [(M, d) for d in (128, 512, 2048) for M in (1, 37, 264)]
RATES = [0.0, 0.1, 0.5]


def rnd(*shape, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(torch.bfloat16)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def to_bf16(x32):
    """numpy float32 -> torch bf16, round-to-nearest-even (the one rounding of the kernels' stores)"""
    return torch.from_numpy(np.ascontiguousarray(x32, dtype=np.float32)).to(torch.bfloat16)


def f32(t):
    return t.float().cpu().numpy()


def _ln_buffers(M, d, fill=None):
    y = torch.empty(M, d, dtype=torch.bfloat16, device=DEV)
    mean, rstd = torch.empty(M, dtype=torch.float32, device=DEV), torch.empty(M, dtype=torch.float32, device=DEV)
    if fill is not None:
        for t in (y, mean, rstd):
            t.fill_(fill)
    return y, mean, rstd


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("M,d", SHAPES)
def test_dropout_add_ln(M, d, rate):
    thresh = dref.threshold(rate)
    g, b = rnd(d, seed=3).add(1).to(DEV), rnd(d, scale=0.1, seed=4).to(DEV)
    # (1) a = 1, residual = 0: the output IS the mask, 0 or bf16(scale), at the restated positions
    x = torch.empty(M, d, dtype=torch.bfloat16, device=DEV)
    y, mean, rstd = _ln_buffers(M, d)
    dh.dropout_add_ln(torch.ones(M, d, dtype=torch.bfloat16, device=DEV), torch.zeros(M, d, dtype=torch.bfloat16, device=DEV), x,
                      g, b, y, mean, rstd, M, d, KEY, thresh)
    assert torch.equal(bits(x), bits(to_bf16(dref.mask(KEY, thresh, (M, d)))))
    # (2) random inputs: one fp32 product, one sum, one rounding; the LayerNorm is layernorm_fwd's of the stored row
    a, res = rnd(M, d, seed=1), rnd(M, d, scale=2.0, seed=2)
    dh.dropout_add_ln(a.to(DEV), res.to(DEV), x, g, b, y, mean, rstd, M, d, KEY, thresh)
    ref = to_bf16(f32(res) + dref.drop(f32(a), KEY, thresh))
    assert torch.equal(bits(x), bits(ref))
    y2, mean2, rstd2 = _ln_buffers(M, d)
    dh.layernorm_fwd(x, g, b, y2, mean2, rstd2, M, d)
    assert torch.equal(bits(y), bits(y2)) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    if thresh == 0:
        assert torch.equal(bits(x), bits((a.float() + res.float()).to(torch.bfloat16)))
    else:
        dropped = ~dref.keep(KEY, thresh, M * d).reshape(M, d)
        assert dropped.any() and torch.equal(bits(x)[torch.from_numpy(dropped)], bits(res)[torch.from_numpy(dropped)])
    # (3) gamma = None: x_out only, the LayerNorm outputs are not touched
    x3 = torch.empty(M, d, dtype=torch.bfloat16, device=DEV)
    y3, mean3, rstd3 = _ln_buffers(M, d, fill=float("nan"))
    dh.dropout_add_ln(a.to(DEV), res.to(DEV), x3, None, None, y3, mean3, rstd3, M, d, KEY, thresh)
    assert torch.equal(bits(x3), bits(ref))
    assert bool(torch.isnan(y3).all()) and bool(torch.isnan(mean3).all()) and bool(torch.isnan(rstd3).all())


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("M,d", SHAPES)
def test_dropout_bwd(M, d, rate):
    thresh = dref.threshold(rate)
    guard = 2
    dx = rnd(M + guard, d, seed=5).to(DEV)
    dy = torch.full((M + guard, d), 7.0, dtype=torch.bfloat16, device=DEV)
    dh.dropout_bwd(dx, dy, M, d, KEY, thresh)
    assert torch.equal(bits(dy[:M]), bits(to_bf16(dref.drop(f32(dx[:M]), KEY, thresh))))
    assert bool((dy[M:] == 7.0).all())                       # nothing past M * d is written
    if thresh == 0:
        assert torch.equal(bits(dy[:M]), bits(dx[:M]))


def _embed_case():
    B, S, d, V = 3, 24, 128, 50
    g = torch.Generator().manual_seed(1)
    tok = torch.randint(0, V - 10, (B, S), generator=g, dtype=torch.int32)      # ids 40..49 stay absent
    tok[:, -7:] = 5                                                              # repeated ids
    tok[1, :3] = tok[0, :3]
    return B, S, d, V, tok, rnd(V, d, scale=0.02, seed=2), rnd(S, d, scale=0.01, seed=3)


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_embed_fwd_dropout(rate):
    B, S, d, V, tok, wte, wpe = _embed_case()
    thresh, k0, k1 = dref.threshold(rate), KEY, KEY ^ 0xFFFF
    x = torch.empty(B * S, d, dtype=torch.bfloat16, device=DEV)
    dh.embed_fwd_dropout(tok.to(DEV), wte.to(DEV), wpe.to(DEV), x, S, d, V, k0, k1, thresh)
    pos = dref.drop(f32(wpe), k1, thresh)                                        # [S, d]: one mask for every batch row
    ref = dref.drop(f32(wte)[tok.long().numpy()], k0, thresh) + pos[None]
    assert torch.equal(bits(x.view(B, S, d)), bits(to_bf16(ref)))
    # the positional mask is shared over the batch: with a zero token table every batch row is the same dropped wpe
    dh.embed_fwd_dropout(tok.to(DEV), torch.zeros_like(wte).to(DEV), wpe.to(DEV), x, S, d, V, k0, k1, thresh)
    xb = x.view(B, S, d)
    assert torch.equal(bits(xb[0]), bits(to_bf16(pos))) and torch.equal(bits(xb[1]), bits(xb[0])) and torch.equal(bits(xb[2]), bits(xb[0]))
    # threshold 0 is the undropped kernel
    x0, x1 = torch.empty_like(x), torch.empty_like(x)
    dh.embed_fwd_dropout(tok.to(DEV), wte.to(DEV), wpe.to(DEV), x0, S, d, V, k0, k1, 0)
    dh.embed_fwd(tok.to(DEV), wte.to(DEV), wpe.to(DEV), x1, S, d, V)
    assert torch.equal(bits(x0), bits(x1))


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_embed_bwd_dropout(rate):
    """dwte / dwpe against float64 within the tolerances of test_kernels_gpu.py::test_embed_fwd_bwd (rtol 1e-5, atol 1e-5)"""
    B, S, d, V, tok, _, _ = _embed_case()
    thresh, k0, k1 = dref.threshold(rate), KEY, KEY ^ 0xFFFF
    dx = rnd(B * S, d, seed=4)
    n = B * S
    st = torch.empty(n, dtype=torch.int32, device=DEV)
    perm = torch.empty(n, dtype=torch.int32, device=DEV)
    dh.sort_tokens(tok.view(-1).to(DEV), st, perm, n, V, torch.empty(dh.sort_tokens_workspace_bytes(n), dtype=torch.uint8, device=DEV))
    outs = []
    for _ in range(2):
        dwte = torch.full((V, d), float("nan"), dtype=torch.float32, device=DEV)       # must be overwritten, zeros for absent ids
        dwpe = torch.full((S, d), float("nan"), dtype=torch.float32, device=DEV)
        dh.embed_bwd_dropout(st, perm, dx.to(DEV), dwte, dwpe, B, S, d, V,
                             torch.empty(dh.embed_bwd_workspace_bytes(B, S, d), dtype=torch.uint8, device=DEV), k0, k1, thresh)
        outs.append((dwte.cpu(), dwpe.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])     # no atomics: equal bits
    m0 = dref.mask(k0, thresh, (n, d)).astype(np.float64)
    m1 = dref.mask(k1, thresh, (S, d)).astype(np.float64)
    dx64 = dx.double().numpy()
    ref_wte = np.zeros((V, d))
    np.add.at(ref_wte, tok.view(-1).long().numpy(), dx64 * m0)
    ref_wpe = m1 * dx64.reshape(B, S, d).sum(0)
    for got, ref, what in ((outs[0][0], ref_wte, "dwte"), (outs[0][1], ref_wpe, "dwpe")):
        err = np.abs(got.double().numpy() - ref)
        assert (err <= 1e-5 + 1e-5 * np.abs(ref)).all(), (what, float(err.max()))
    absent = sorted(set(range(V)) - set(tok.view(-1).tolist()))
    assert len(absent) >= 10 and bool((outs[0][0][absent] == 0).all())
    assert float(np.abs(ref_wte).max()) > 0 and bool((outs[0][1] == 0).any())              # dropped positional elements are exact zeros


# ------------------------------------------------------------------ engine
def _model(n_embd=256, n_heads=2, B=BATCH, **extra):
    return build(n_embd, n_heads, batch=B, hparams=extra)


@pytest.mark.parametrize("n_embd,n_heads", WIDTHS)
def test_engine_step_vs_masked_fp32_oracle(n_embd, n_heads):
    """loss within 5e-4 relative, worst per-tensor gradient relative L2 <= 4.8e-2 (tests/parity.py check_report) against the fp32
    oracle with the engine's own masks (engine.last_dropout) injected; and the engine is far from the plain oracle"""
    import dalle_step_ref as sref
    from oracle import dalle_oracle as do
    cfg, model, P0, tokens = _model(n_embd, n_heads, embed_dropout=RATE, residual_dropout=RATE)
    eng = model.engine
    loss, _ = step(eng, tokens)
    loss = float(loss.item())
    gh = eng.export_reference(eng.g)
    t = dref.threshold(RATE)
    assert eng.last_dropout == {site: (dref.site_key(0, 0, 0, 0, site), t) for site in range(2 + 2 * NL)}
    masks = dref.engine_masks(eng.last_dropout, BATCH, T + P, n_embd, NL)
    loss_o, go = sref.loss_and_grads(P0, tokens, cfg, dropout=masks)
    worst = max((rel_l2(gh[k], go[k]), k) for k in go)
    _, gp = do.loss_and_grads(P0, tokens, cfg)
    far = max(rel_l2(gh[k], gp[k]) for k in gp)
    print(f"dropout engine (n_embd {n_embd}) vs masked fp32 oracle: loss {loss} {loss_o} rel {abs(loss - loss_o) / abs(loss_o):.3g} "
          f"worst grad {worst}; vs plain oracle {far}", flush=True)
    assert abs(loss - loss_o) <= 5e-4 * abs(loss_o), (loss, loss_o)
    assert worst[0] <= 4.8e-2, worst
    assert far > 0.2, far


def test_keys_zero_or_absent_are_bit_identical():
    out = []
    for extra in ({}, dict(embed_dropout=0, residual_dropout=0.0, dropout_seed=5), dict(embed_dropout=None, residual_dropout=None)):
        _, model, _, tokens = _model(512, 4, **extra)
        assert model.engine.dyd is None
        out.append(step(model.engine, tokens))
        assert model.engine.last_dropout == {}
        del model
        torch.cuda.empty_cache()
    for loss, g in out[1:]:
        assert torch.equal(loss, out[0][0]) and torch.equal(g, out[0][1])


@pytest.mark.parametrize("n_embd,n_heads", WIDTHS)
def test_recompute_grad_with_dropout_equals_stored_activations(n_embd, n_heads):
    res = []
    for rc in (False, True):
        _, model, _, tokens = _model(n_embd, n_heads, embed_dropout=RATE, residual_dropout=RATE, recompute_grad=rc)
        res.append(step(model.engine, tokens))
        del model
        torch.cuda.empty_cache()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_microbatches_and_steps_draw_their_own_masks():
    _, model, _, tokens = _model(256, 2, B=1, embed_dropout=RATE, residual_dropout=RATE, dropout_seed=11, num_microbatches=2)
    eng = model.engine
    seen, forward = [], eng.forward

    def recording(*a, **k):
        r = forward(*a, **k)
        seen.append((dict(eng.last_dropout), eng.X[0].clone()))
        return r
    eng.forward = recording
    tok = torch.from_numpy(tokens[:1]).cuda().repeat(2, 1)              # both micro-batches carry the SAME tokens
    eng.train_step(tok)
    eng.train_step(tok)
    torch.cuda.synchronize()
    t = dref.threshold(RATE)
    want = [{site: (dref.site_key(11, step, mb, 0, site), t) for site in range(2 + 2 * NL)} for step in (0, 1) for mb in (0, 1)]
    assert [s[0] for s in seen] == want
    keys = [k for s in seen for k, _ in s[0].values()]
    assert len(set(keys)) == len(keys)
    for i in range(4):
        for j in range(i + 1, 4):
            assert not torch.equal(seen[i][1], seen[j][1]), (i, j)       # same tokens, other masks: other embeddings
    # the same (step, microbatch) restates the same masks
    eng.forward = forward
    eng.global_step = 0
    eng.forward(tok[:1], need_grad=True)
    assert eng.last_dropout == want[0]


def test_evaluation_logits_and_sampling_ignore_the_keys():
    outs = []
    for extra in ({}, dict(embed_dropout=RATE, residual_dropout=RATE)):
        _, model, P0, tokens = _model(256, 2, **extra)
        eng = model.engine
        tok = torch.from_numpy(tokens).cuda()
        # a (dropped) training step first, then the starting weights again: what follows must not inherit the step's masks
        eng.train_step(tok)
        assert bool(eng.last_dropout) == bool(extra)
        eng.load_reference_params(P0)
        loss = eng.forward(tok, need_grad=False).clone()
        assert eng.last_dropout == {}
        logits = eng.logits().clone()
        model.mode = "train"
        l2, _, lg2 = model.forward({"tokens": tok}, return_logits=True)       # train mode with return_logits: the evaluation path
        text = tok[:, :T].contiguous()
        a = eng.sample_image_tokens(text, temperature=1.0, top_k=8, seed=3)
        b = eng.sample_image_tokens(text, temperature=1.0, top_k=8, seed=3, kv_cache=False)
        outs.append((loss, logits, l2.clone(), lg2.clone(), a.clone(), b.clone()))
        del model, eng
        torch.cuda.empty_cache()
    for x, y in zip(*outs):
        assert torch.equal(x, y)


def test_resume_continues_the_mask_sequence():
    """two steps, state_dict, two more steps == load + two steps: weights and optimizer state, bit for bit"""
    extra = dict(embed_dropout=RATE, residual_dropout=RATE, dropout_seed=3)
    _, model, _, tokens = _model(256, 2, **extra)
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    for _ in range(2):
        eng.train_step(tok)
    sd = eng.state_dict()
    for _ in range(2):
        eng.train_step(tok)
    torch.cuda.synchronize()
    end = (eng.p.clone(), eng.m.clone(), eng.v.clone(), eng.global_step)
    del model, eng
    _, model, _, _ = _model(256, 2, **extra)
    eng = model.engine
    eng.load_state_dict(sd)
    for _ in range(2):
        eng.train_step(tok)
    torch.cuda.synchronize()
    assert eng.global_step == end[3] == 4
    assert torch.equal(eng.p, end[0]) and torch.equal(eng.m, end[1]) and torch.equal(eng.v, end[2])
    # ... and the masks matter to the weights: the same four steps without dropout end elsewhere
    _, plain, _, _ = _model(256, 2)
    for _ in range(4):
        plain.engine.train_step(tok)
    torch.cuda.synchronize()
    assert not torch.equal(plain.engine.p, end[0])
