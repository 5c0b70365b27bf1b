"""Rotary position embeddings on the MI355X: dmi_rope_qk / dmi_rope_qk_decode against float64, the engine's train step against
the fp32 step oracle with the same table (tests/dalle_step_ref.py), the unset key, recompute_grad, the decode step and the samplers, checkpoints."""
import numpy as np
import pytest
import torch

from engine_case import P, PATTERNS, T, build, decode_worst, samplers_agree, step, step_pair
from parity import rel_l2

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ kernels
KS, KH, KB = 40, 2, 2            # S = 40: no multiple of a block's four rows times anything; T = 4 caption + 6 x 6 image positions


def _table(hd, scheme="axial"):
    from src.dalle_mtf.rotary import rotary_table
    return rotary_table(scheme, 4, 36, hd)


def _inputs(rows, hd, seed):
    """bf16 [rows + 1, 3 H hd] (the last row is the guard), standard normal with a few +-large and zero entries"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows + 1, 3 * KH * hd, generator=g)
    flat = x.view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:96]
    flat[idx[:24]] = 3.0e4
    flat[idx[24:48]] = -1.0e6
    flat[idx[48:]] = 0.0
    return x.to(torch.bfloat16)


def _tol(y64, x64, H, hd):
    """per element 2^-8 |y64| + 2^-20 (|x0| + |x1|): one bf16 rounding (half a spacing of 2^-7) of an fp32 result whose own error
    is a few fp32 ulps of the operands; x0, x1 = the element's pair"""
    w = 2 * H * hd
    pair = np.abs(x64[:, :w]).reshape(x64.shape[0], -1, 2).sum(-1, keepdims=True).repeat(2, -1).reshape(x64.shape[0], w)
    return 2.0 ** -8 * np.abs(y64[:, :w]) + 2.0 ** -20 * pair


def _run(x, cs, rows, hd, inverse):
    import dalle_hip as dh
    buf = x.clone().cuda()
    dh.rope_qk(buf, cs, rows, KS, KH, hd, inverse=inverse)
    torch.cuda.synchronize()
    return buf.cpu()


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("rows", [KB * KS, 3 * KS + 8])
@pytest.mark.parametrize("hd", [64, 128])
def test_rope_qk_vs_float64(hd, rows, inverse):
    import rotary_ref as rref
    table = _table(hd)
    cs = torch.from_numpy(table).cuda()
    x = _inputs(rows, hd, seed=hd + rows)
    y = _run(x, cs, rows, hd, inverse)
    w = 2 * KH * hd
    assert torch.equal(y[:rows, w:].view(torch.int16), x[:rows, w:].view(torch.int16))      # v: bit-identical
    assert torch.equal(y[rows].view(torch.int16), x[rows].view(torch.int16))                # the guard row behind the buffer
    x64 = x[:rows].double().numpy()
    y64 = rref.rope64(x64, table, KH, hd, KS, inverse=inverse)
    err = np.abs(y[:rows, :w].double().numpy() - y64[:, :w])
    tol = _tol(y64, x64, KH, hd)
    print(f"rope_qk hd {hd} rows {rows} inverse {inverse}: worst err / tol {float((err / np.maximum(tol, 1e-300)).max()):.3f}", flush=True)
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    assert not np.array_equal(y[:rows, :w].double().numpy(), x64[:, :w])                   # it did rotate


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_qk_inverse_is_the_adjoint(hd):
    """<rope(x), y> = <x, rope_inverse(y)> in float64 over the kernel's outputs, within what the per-element tolerance allows:
    sum tol(rope x) |y| + sum |x| tol(rope_inverse y) (the exact rotations are each other's transposes)"""
    import rotary_ref as rref
    rows, w = KB * KS, 2 * KH * hd
    table = _table(hd)
    cs = torch.from_numpy(table).cuda()
    g = torch.Generator().manual_seed(7 + hd)
    x = torch.randn(rows + 1, 3 * KH * hd, generator=g).to(torch.bfloat16)
    y = torch.randn(rows + 1, 3 * KH * hd, generator=g).to(torch.bfloat16)
    rx = _run(x, cs, rows, hd, False)[:rows, :w].double().numpy()
    ry = _run(y, cs, rows, hd, True)[:rows, :w].double().numpy()
    x64, y64 = x[:rows].double().numpy(), y[:rows].double().numpy()
    lhs, rhs = float((rx * y64[:, :w]).sum()), float((x64[:, :w] * ry).sum())
    bound = float((_tol(rref.rope64(x64, table, KH, hd, KS), x64, KH, hd) * np.abs(y64[:, :w])).sum()
                  + (np.abs(x64[:, :w]) * _tol(rref.rope64(y64, table, KH, hd, KS, inverse=True), y64, KH, hd)).sum())
    print(f"adjoint hd {hd}: {lhs} vs {rhs}, |diff| {abs(lhs - rhs):.3e} <= {bound:.3e}", flush=True)
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    assert abs(lhs) > 0


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_qk_round_trip(hd):
    """rope_inverse(rope(x)) is within two bf16 roundings of x.  With r = |(x0, x1)|_2: the first rounding moves the rotated pair
    by at most 2^-8 r per element, the exact inverse rotation keeps that length, the second rounding adds 2^-8 |z| <=
    2^-8 (1 + 2^-7) r; the two fp32 evaluations add 2^-19 r."""
    rows, w = KB * KS, 2 * KH * hd
    cs = torch.from_numpy(_table(hd)).cuda()
    x = _inputs(rows, hd, seed=99 + hd)
    z = _run(_run(x, cs, rows, hd, False), cs, rows, hd, True)
    assert torch.equal(z[:, w:].view(torch.int16), x[:, w:].view(torch.int16))
    x64 = x[:rows, :w].double().numpy()
    r = np.sqrt((x64.reshape(rows, -1, 2) ** 2).sum(-1, keepdims=True)).repeat(2, -1).reshape(rows, w)
    err = np.abs(z[:rows, :w].double().numpy() - x64)
    tol = (2.0 ** -8 * (2 + 2.0 ** -7) + 2.0 ** -19) * r
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_qk_decode_equals_the_rows_of_the_full_kernel(hd):
    import dalle_hip as dh
    B, ld = 3, 3 * KH * hd
    cs = torch.from_numpy(_table(hd, "1d")).cuda()
    g = torch.Generator().manual_seed(hd)
    fresh = torch.randn(B, ld, generator=g).to(torch.bfloat16).cuda()
    guard = torch.randn(B + 1, ld, generator=g).to(torch.bfloat16).cuda()      # decode buffers with a guard row
    pos_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    for pos, by_dev in ((0, False), (KS - 1, False), (0, True), (17, True), (KS - 1, True)):
        full = torch.zeros(B * KS, ld, dtype=torch.bfloat16, device="cuda")
        full[pos::KS] = fresh
        dh.rope_qk(full, cs, B * KS, KS, KH, hd)
        buf = guard.clone()
        buf[:B] = fresh
        if by_dev:
            pos_dev.fill_(pos)
            dh.rope_qk_decode(buf, cs, B, KS, KH, hd, pos=12345, pos_dev=pos_dev)      # the by-value position is ignored
        else:
            dh.rope_qk_decode(buf, cs, B, KS, KH, hd, pos=pos)
        torch.cuda.synchronize()
        assert torch.equal(buf[:B].view(torch.int16), full[pos::KS].view(torch.int16)), (pos, by_dev)
        assert torch.equal(buf[B].view(torch.int16), guard[B].view(torch.int16))
        if pos:
            assert not torch.equal(buf[:B], fresh)
    for bad in (KS, -1):
        pos_dev.fill_(bad)
        buf = fresh.clone()
        dh.rope_qk_decode(buf, cs, B, KS, KH, hd, pos_dev=pos_dev)
        torch.cuda.synchronize()
        assert torch.equal(buf.view(torch.int16), fresh.view(torch.int16)), bad


# ------------------------------------------------------------------ engine
def _setup(rotary="axial", hparams=None, **kw):
    return build(hparams=dict(hparams or {}, rotary_emb=rotary), **kw)


@pytest.mark.parametrize("n_embd,scheme,patterns", [(256, "axial", None), (128, "1d", None), (256, "axial", PATTERNS)],
                         ids=["hd128-axial", "hd64-1d", "hd128-axial-masked"])
def test_engine_step_vs_rotated_fp32_oracle(n_embd, scheme, patterns):
    """the project's causal-step bounds (tests/parity.py check_report): loss 5e-4 relative, worst gradient tensor 4.8e-2 relative L2
    -- the rotation adds one bf16 rounding of q and k, the size of the rounding the QKV output already carries"""
    import dalle_step_ref as sref
    from src.dalle_mtf.masks import layer_masks
    from src.dalle_mtf.rotary import rotary_table
    cfg, model, P0, tokens = _setup(scheme, width=n_embd, hparams=dict(attention_pattern=patterns or "absent"))
    eng = model.engine
    assert eng.rotary == scheme and eng.rope_cs is not None and tuple(eng.rope_cs.shape) == (T + P, eng.hd // 2, 2)
    assert (patterns is None) == all(p is None for p in eng.attn_plan)
    loss = float(step(eng, tokens)[0].item())
    gh = eng.export_reference(eng.g)
    masks = layer_masks(patterns, cfg.n_layers, T, P) if patterns is not None else None
    loss_o, go = sref.loss_and_grads(P0, tokens, cfg, table=rotary_table(scheme, T, P, eng.hd), masks=masks)
    worst = max((rel_l2(gh[k], go[k]), k) for k in go)
    print(f"rotary {scheme} n_embd {n_embd} masked {patterns is not None}: loss {loss} oracle {loss_o} worst grad {worst}", flush=True)
    assert abs(loss - loss_o) <= 5e-4 * abs(loss_o), (loss, loss_o)
    assert worst[0] <= 4.8e-2, worst


def test_the_rotation_is_live():
    """attn/q and attn/k scaled by 2 (chosen on the CPU: the rotary and the rotary-off fp32 oracles then differ by 1.34 .. 1.43
    relative L2 on those tensors, asserted > 0.2 below): the engine's q / k gradients are at least ten times farther from the
    rotary-off oracle than from the rotary one"""
    import dalle_step_ref as sref
    from oracle import dalle_oracle as do
    from src.dalle_mtf.rotary import rotary_table
    cfg, model, P0, tokens = _setup()
    eng = model.engine
    P0 = {k: (v * np.float32(2.0) if k.endswith(("attn/q", "attn/k")) else v) for k, v in P0.items()}
    eng.load_reference_params(P0)
    step(eng, tokens)
    gh = eng.export_reference(eng.g)
    _, g_on = sref.loss_and_grads(P0, tokens, cfg, table=rotary_table("axial", T, P, eng.hd))
    _, g_off = do.loss_and_grads(P0, tokens, cfg)
    for k in (k for k in g_on if k.endswith(("attn/q", "attn/k"))):
        assert rel_l2(g_on[k], g_off[k]) > 0.2, k
        near, far = rel_l2(gh[k], g_on[k]), rel_l2(gh[k], g_off[k])
        print(f"live {k}: vs rotary oracle {near:.4f}, vs rotary-off oracle {far:.4f}", flush=True)
        assert far >= 10 * near, (k, near, far)


def test_off_is_off():
    """the key absent, None and False: bit-identical loss and flat gradient, no table"""
    out = []
    for rotary in ("absent", None, False):
        _, model, _, tokens = _setup(rotary)
        eng = model.engine
        assert eng.rotary is None and eng.rope_cs is None
        assert "rotary_emb" not in eng.state_dict()
        out.append(step(eng, tokens))
        del model, eng
        torch.cuda.empty_cache()
    for loss, g in out[1:]:
        assert torch.equal(loss, out[0][0]) and torch.equal(g, out[0][1])
    _, model, _, tokens = _setup()         # ... and on is not off
    assert not torch.equal(step(model.engine, tokens)[0], out[0][0])


def test_recompute_grad_with_rotary_equals_stored_activations():
    res = step_pair(lambda rc: _setup(hparams=dict(recompute_grad=rc))[1::2])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


def test_rotary_decode_logits_and_samplers():
    """decode-step logits (graph and eager) against the full forward at every image position: the existing 3e-2 relative bound;
    graph-replayed, host-launched and unfused-draw samplers give equal tokens; a guided sample equals its decode_graph=False twin"""
    _, model, _, tokens = _setup()
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    for graph in (True, False):
        worst = decode_worst(eng, tok, graph=graph)
        print(f"rotary decode (graph={graph}) vs full forward logits: worst relative {worst}", flush=True)
        assert worst <= 3e-2, (graph, worst)
    samplers_agree(eng, tok[:, :T].contiguous())


def test_checkpoint_records_and_checks_the_scheme():
    _, model, _, tokens = _setup()
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    eng.forward(tok, need_grad=False)
    want = eng.logits().clone()
    sd = eng.state_dict()
    assert sd["rotary_emb"] == "axial" and sd["rotary_base"] == 10000.0
    del model, eng
    for kw, word in ((dict(rotary="absent"), "no rotary"), (dict(rotary="1d"), "'1d'"), (dict(hparams=dict(rotary_base=500.0)), "500")):
        _, other, _, _ = _setup(**kw)
        with pytest.raises(ValueError, match="rotary") as e:
            other.engine.load_state_dict(sd)
        assert word in str(e.value) and "'axial'" in str(e.value), str(e.value)
        plain = {k: v for k, v in sd.items() if k not in ("rotary_emb", "rotary_base")}      # a checkpoint from before the key
        if kw.get("rotary") == "absent":
            other.engine.load_state_dict(plain)
        else:
            with pytest.raises(ValueError, match="no rotary"):
                other.engine.load_state_dict(plain)
        del other
        torch.cuda.empty_cache()
    _, same, _, _ = _setup(seed=7)           # other initial weights: the logits below are the checkpoint's
    same.engine.load_state_dict(sd)
    same.engine.forward(tok, need_grad=False)
    assert torch.equal(same.engine.logits(), want)
