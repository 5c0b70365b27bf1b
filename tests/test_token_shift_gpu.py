"""Token shift on the MI355X: dmi_token_shift / dmi_token_shift_decode bit for bit against the float64 reference
(tests/token_shift_ref.py), the engine's train step against the shifted fp32 oracle (tests/dalle_step_ref.py), the unset key, recompute_grad, the decode
step with its history and the samplers, checkpoints."""
import pytest
import torch

from engine_case import P, PATTERNS, T, TV, build, decode_worst, inputs, samplers_agree, step, step_pair
from parity import rel_l2

pytestmark = pytest.mark.gpu
G = 16

# ------------------------------------------------------------------ kernels
KB = 3                            # sequences; T = 4 caption + 6 x 6 image positions: S = 40
SHAPES = [(4, 6, 32), (4, 6, 96), (4, 6, 512), (1, 6, 32), (4, 1, 32)]     # (T, G, d)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(rows, d, seed):
    """bf16 [rows, d]: standard normal with a few +-large values, zeros and -0"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, d, generator=g)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:96]
    flat[idx[:24]] = 3.0e4
    flat[idx[24:48]] = -1.0e6
    flat[idx[48:72]] = 0.0
    flat[idx[72:]] = -0.0
    return x.to(torch.bfloat16)


def _guarded(rows, width, seed):
    """a device buffer of rows + 1 rows of noise: the kernel's output and the guard row behind it"""
    g = torch.Generator().manual_seed(1000 + seed)
    return torch.randn(rows + 1, width, generator=g).to(torch.bfloat16).cuda()


def _want(x, Tk, Gk, inverse=False):
    """shift64 of the bf16 values, back in bf16: every value is one of the inputs or +0, so the cast is exact"""
    import token_shift_ref as tref
    return torch.from_numpy(tref.shift64(x.double().numpy(), Tk, Gk, inverse=inverse)).to(torch.bfloat16)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("Tk,Gk,d", SHAPES)
def test_token_shift_equals_shift64_bit_for_bit(Tk, Gk, d, inverse):
    import dalle_hip as dh
    S = Tk + Gk * Gk
    rows = KB * S
    x = _inputs(rows, d, seed=d + Tk + Gk)
    y = _guarded(rows, d, seed=d)
    guard = y[rows].clone()
    dh.token_shift(x.cuda(), y, rows, S, Tk, Gk, d, inverse=inverse)
    torch.cuda.synchronize()
    want = _want(x, Tk, Gk, inverse)
    assert torch.equal(_bits(y[:rows].cpu()), _bits(want))                     # copies and +0, nothing else
    assert torch.equal(_bits(y[rows]), _bits(guard))                           # the guard row behind y
    assert not torch.equal(_bits(want), _bits(x))                              # it did shift


@pytest.mark.parametrize("Tk,Gk,d", SHAPES)
def test_token_shift_writes_the_history(Tk, Gk, d):
    import dalle_hip as dh
    S = Tk + Gk * Gk
    rows = KB * S
    x = _inputs(rows, d, seed=7 + d + Tk + Gk)
    y, hist = _guarded(rows, d, seed=1), _guarded(rows, d // 2, seed=2)
    gy, gh = y[rows].clone(), hist[rows].clone()
    dh.token_shift(x.cuda(), y, rows, S, Tk, Gk, d, hist=hist)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y[:rows].cpu()), _bits(_want(x, Tk, Gk)))
    assert torch.equal(_bits(hist[:rows].cpu()), _bits(x[:, :d // 2]))
    assert torch.equal(_bits(y[rows]), _bits(gy)) and torch.equal(_bits(hist[rows]), _bits(gh))


@pytest.mark.parametrize("Tk,Gk,d", SHAPES)
def test_token_shift_inverse_is_the_adjoint(Tk, Gk, d):
    """sum shift(x) . y == sum x . shift^T(y) exactly, in float64 over the kernels' outputs: both sides are sums of the same
    products.  A product of two bf16 values is exact in float64, and math.fsum returns the correctly rounded sum of its terms, which
    does not depend on their order -- so equal multisets of terms give equal floats, and anything else shows."""
    import math
    import dalle_hip as dh
    S = Tk + Gk * Gk
    rows = KB * S
    g = torch.Generator().manual_seed(11 + d)
    x = torch.randn(rows, d, generator=g).to(torch.bfloat16)
    y = torch.randn(rows, d, generator=g).to(torch.bfloat16)
    sx = torch.empty(rows, d, dtype=torch.bfloat16, device="cuda")
    sty = torch.empty(rows, d, dtype=torch.bfloat16, device="cuda")
    dh.token_shift(x.cuda(), sx, rows, S, Tk, Gk, d)
    dh.token_shift(y.cuda(), sty, rows, S, Tk, Gk, d, inverse=True)
    torch.cuda.synchronize()
    lhs = math.fsum((sx.cpu().double().numpy() * y.double().numpy()).ravel())
    rhs = math.fsum((x.double().numpy() * sty.cpu().double().numpy()).ravel())
    print(f"adjoint T {Tk} G {Gk} d {d}: {lhs!r} vs {rhs!r}", flush=True)
    assert lhs == rhs, (lhs, rhs)
    assert abs(lhs) > 0


@pytest.mark.parametrize("d", [32, 512])
def test_token_shift_decode_equals_the_rows_of_the_full_kernel(d):
    import dalle_hip as dh
    Tk, Gk = 4, 6
    S = Tk + Gk * Gk
    B = KB
    x = _inputs(B * S, d, seed=3 + d).cuda()
    full = torch.empty(B * S, d, dtype=torch.bfloat16, device="cuda")
    hist0 = torch.empty(B * S, d // 2, dtype=torch.bfloat16, device="cuda")
    dh.token_shift(x, full, B * S, S, Tk, Gk, d, hist=hist0)
    full, x3 = full.view(B, S, d), x.view(B, S, d)
    pos_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    g = torch.Generator().manual_seed(5)
    noise = torch.randn(B, d // 2, generator=g).to(torch.bfloat16).cuda()
    for pos in (0, Tk - 1, Tk, Tk + 1, Tk + Gk - 1, Tk + Gk, S - 1):
        for by_dev in (False, True):
            hist = torch.cat([hist0.view(B, S, d // 2), torch.zeros(1, S, d // 2, dtype=torch.bfloat16, device="cuda")]).contiguous()
            hist[:B, pos] = noise                                  # the step itself must write this row
            before = hist.clone()
            y = _guarded(B, d, seed=pos)
            gy = y[B].clone()
            xin = x3[:, pos].contiguous()
            if by_dev:
                pos_dev.fill_(pos)
                dh.token_shift_decode(xin, hist, y, B, S, Tk, Gk, d, pos=12345, pos_dev=pos_dev)      # the by-value position is ignored
            else:
                dh.token_shift_decode(xin, hist, y, B, S, Tk, Gk, d, pos=pos)
            torch.cuda.synchronize()
            assert torch.equal(_bits(y[:B]), _bits(full[:, pos])), (pos, by_dev)
            assert torch.equal(_bits(y[B]), _bits(gy))
            assert torch.equal(_bits(hist[:B, pos]), _bits(x3[:, pos, :d // 2])), (pos, by_dev)
            keep = torch.ones(B + 1, S, dtype=torch.bool, device="cuda")
            keep[:B, pos] = False
            assert torch.equal(_bits(hist[keep]), _bits(before[keep])), (pos, by_dev)                  # every other row, and the guard sequence
    for bad in (-1, S):
        pos_dev.fill_(bad)
        hist = hist0.view(B, S, d // 2).clone()
        y = _guarded(B, d, seed=77)
        y0 = y.clone()
        dh.token_shift_decode(x3[:, 0].contiguous(), hist, y, B, S, Tk, Gk, d, pos_dev=pos_dev)
        torch.cuda.synchronize()
        assert torch.equal(_bits(y), _bits(y0)) and torch.equal(_bits(hist), _bits(hist0.view(B, S, d // 2))), bad


# ------------------------------------------------------------------ engine
def _setup(shift=True, hparams=None, **kw):
    return build(hparams=dict(hparams or {}, token_shift=shift), **kw)


_ORACLE = {}


def _oracle(n_embd, shift):
    """the fp32 oracle's (loss, gradients) at the default setup (3 layers, 2 heads, causal, no rotation): computed once per arm
    and shared by the tests that need it"""
    key = (n_embd, shift)
    if key not in _ORACLE:
        import dalle_step_ref as sref
        cfg, P0, tokens = inputs(n_embd)
        _ORACLE[key] = sref.loss_and_grads(P0, tokens, cfg, token_shift=shift)
    return _ORACLE[key]


@pytest.mark.parametrize("n_embd,n_heads,n_layers,patterns,rotary",
                         [(256, 2, 3, None, None), (128, 2, 3, None, None), (256, 2, 3, PATTERNS, "axial"), (512, 4, 2, None, None)],
                         ids=["hd128", "hd64", "hd128-masked-axial", "n_embd512"])
def test_engine_step_vs_shifted_fp32_oracle(n_embd, n_heads, n_layers, patterns, rotary):
    """the project's causal-step bounds (tests/parity.py check_report): loss 5e-4 relative, worst gradient tensor 4.8e-2 relative L2
    -- the shift copies, it adds no rounding"""
    import dalle_step_ref as sref
    from src.dalle_mtf.masks import layer_masks
    from src.dalle_mtf.rotary import rotary_table
    cfg, model, P0, tokens = _setup(width=n_embd, heads=n_heads, layers=n_layers,
                                    hparams=dict(attention_pattern=patterns or "absent", rotary_emb=rotary or "absent"))
    eng = model.engine
    assert eng.token_shift is True and eng.G == G and tuple(eng.shift_tmp.shape) == (eng.M, n_embd)
    assert not eng.fuse_lnbwd and not eng.lnb_batch and not eng._d_o_chained()
    if n_embd == 512:
        print(f"n_embd 512 LayerNorm forms: fuse_ln {eng.fuse_ln} fuse_ln1 {eng.fuse_ln1} fuse_lnbwd {eng.fuse_lnbwd} "
              f"lnb_batch {eng.lnb_batch}", flush=True)
    loss = float(step(eng, tokens)[0].item())
    gh = eng.export_reference(eng.g)
    if patterns is None and rotary is None and n_layers == 3:
        loss_o, go = _oracle(n_embd, True)
    else:
        masks = layer_masks(patterns, cfg.n_layers, T, P) if patterns is not None else None
        table = rotary_table(rotary, T, P, eng.hd) if rotary is not None else None
        loss_o, go = sref.loss_and_grads(P0, tokens, cfg, token_shift=True, table=table, masks=masks)
    worst = max((rel_l2(gh[k], go[k]), k) for k in go)
    print(f"token_shift n_embd {n_embd} masked {patterns is not None} rotary {rotary}: loss {loss} oracle {loss_o} worst grad {worst}",
          flush=True)
    assert abs(loss - loss_o) <= 5e-4 * abs(loss_o), (loss, loss_o)
    assert worst[0] <= 4.8e-2, worst


@pytest.mark.parametrize("n_embd", [256, 128])
def test_the_shift_is_live(n_embd):
    """on the tensors the shifted rows feed (q, k, v and FFN-1's kernel) the shift-on and shift-off fp32 oracles differ by more
    than 0.2 relative L2 (0.25 .. 1.08 on the CPU at this setup), and the engine's gradient is more than 0.15 away from the
    shift-off one; the loss moves by 1.3e-3 relative only, so the gradients are what is asserted"""
    _, model, _, tokens = _setup(width=n_embd)
    eng = model.engine
    step(eng, tokens)
    gh = eng.export_reference(eng.g)
    _, g_on = _oracle(n_embd, True)
    _, g_off = _oracle(n_embd, False)
    keys = [k for k in g_on if k.endswith(("attn/q", "attn/k", "attn/v", "mlp/mlp_linear_1/kernel"))]
    assert len(keys) == 4 * 3
    for k in keys:
        apart, far = rel_l2(g_on[k], g_off[k]), rel_l2(gh[k], g_off[k])
        print(f"live {k}: oracles apart {apart:.4f}, engine vs shift-off oracle {far:.4f}", flush=True)
        assert apart > 0.2, (k, apart)
        assert far > 0.15, (k, far)


def test_off_is_off():
    """the key absent, None and False: bit-identical loss and flat gradient, no shift buffers, nothing in the checkpoint"""
    out = []
    for shift in ("absent", None, False):
        _, model, _, tokens = _setup(shift)
        eng = model.engine
        assert eng.token_shift is False and eng.shift_tmp is None and eng.G is None
        out.append(step(eng, tokens))
        eng._prefill(torch.from_numpy(tokens).cuda())
        eng.decode_step(torch.from_numpy(tokens[:, T - 1].copy()).cuda(), T - 1)
        assert eng._shift_hist is None and "xs" not in eng._dec
        assert "token_shift" not in eng.state_dict()
        del model, eng
        torch.cuda.empty_cache()
    for loss, g in out[1:]:
        assert torch.equal(loss, out[0][0]) and torch.equal(g, out[0][1])
    _, model, _, tokens = _setup()         # ... and on is not off
    loss, g = step(model.engine, tokens)
    assert not torch.equal(loss, out[0][0]) and not torch.equal(g, out[0][1])


def test_recompute_grad_with_token_shift_equals_stored_activations():
    res = step_pair(lambda rc: _setup(hparams=dict(recompute_grad=rc, residual_dropout=0.1, embed_dropout=0.1))[1::2])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().sum()) > 0


def test_token_shift_decode_logits_against_the_full_forward():
    """decode-step logits (graph and eager) at every image position: the existing 3e-2 relative bound against the full forward --
    after a prefill of the true tokens, and after a prefill whose image part is all zeros followed by decode steps fed the true
    tokens from position T - 1 on: then every history row of an image position must come from a decode step"""
    _, model, _, tokens = _setup()
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    blind = tok.clone()
    blind[:, T:] = 0
    for name, fill in (("true tokens", tok), ("image part zero", blind)):
        for graph in (True, False):
            worst = decode_worst(eng, tok, fill=fill, graph=graph)
            print(f"token_shift decode after a prefill of {name} (graph={graph}) vs full forward logits: worst relative {worst}", flush=True)
            assert worst <= 3e-2, (name, graph, worst)
    assert eng._shift_hist is not None and len(eng._shift_hist) == 3 and tuple(eng._shift_hist[0][1].shape) == (2, T + P, 128)


def test_token_shift_samplers_agree():
    """graph-replayed, host-launched and unfused-draw samplers give equal tokens; a guided sample and a sample with an image
    prefix of G + 3 tokens equal their decode_graph=False twins"""
    _, model, _, tokens = _setup()
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    text = tok[:, :T].contiguous()
    samplers_agree(eng, text)
    prefix = (tok[:, T:T + G + 3] - TV).contiguous()
    p1 = eng.sample_image_tokens(text, temperature=1.0, top_k=8, seed=9, image_prefix=prefix)
    p2 = eng.sample_image_tokens(text, temperature=1.0, top_k=8, seed=9, image_prefix=prefix, decode_graph=False)
    assert torch.equal(p1[:, :G + 3], prefix.to(p1.dtype)) and torch.equal(p1, p2)


def test_checkpoint_records_and_checks_the_key():
    _, model, _, tokens = _setup()
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    eng.forward(tok, need_grad=False)
    want = eng.logits().clone()
    sd = eng.state_dict()
    assert sd["token_shift"] is True
    before = {k: v for k, v in sd.items() if k != "token_shift"}         # a checkpoint from before the key
    with pytest.raises(ValueError, match="token_shift") as e:           # ... is a model without the shift
        eng.load_state_dict(before)
    assert "no token shift" in str(e.value) and "token_shift on" in str(e.value), str(e.value)
    del model, eng
    _, off, _, _ = _setup("absent")
    with pytest.raises(ValueError, match="token_shift") as e:
        off.engine.load_state_dict(sd)
    assert "no token shift" in str(e.value) and "token_shift on" in str(e.value), str(e.value)
    off.engine.load_state_dict(before)
    sd_off = off.engine.state_dict()
    assert "token_shift" not in sd_off
    del off
    torch.cuda.empty_cache()
    _, same, _, _ = _setup(seed=7)           # other initial weights: the logits below are the checkpoint's
    with pytest.raises(ValueError, match="token_shift"):
        same.engine.load_state_dict(sd_off)
    same.engine.load_state_dict(sd)
    same.engine.forward(tok, need_grad=False)
    assert torch.equal(same.engine.logits(), want)
