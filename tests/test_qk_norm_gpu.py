"""QK normalisation on the MI355X: dmi_qk_norm_fwd / _bwd / _decode against float64 (tests/qk_norm_ref.py), the engine's train step
against the fp32 step oracle with the normalisation, the unset key, recompute_grad, micro-batches, the optimizers and the weight
average, the decode step and the samplers, checkpoints."""
import numpy as np
import pytest
import torch

import qk_norm_ref as qref
from engine_case import HP, IV, P, PATTERNS, T, TV, build, decode_worst, inputs, samplers_agree, step, step_pair
from parity import rel_l2

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------ kernels
KS, KH = 40, 2                   # S = 40: T = 4 caption + 6 x 6 image positions; rows 80 = two sequences, 128 = more than one pass of
ROWS = (80, 128, 1)              # a small grid's blocks of four rows and no multiple of S, 1 = a block with three idle waves


def _table(hd, scheme="axial"):
    from src.dalle_mtf.rotary import rotary_table
    return rotary_table(scheme, 4, 36, hd)


def _inputs(rows, hd, seed):
    """bf16 [rows + 1, 3 H hd] (the last row is the guard): standard normal with a few +-3e4 and 1e-20 entries, exact zeros and one
    all-zero head (row 0, q head 0)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows + 1, 3 * KH * hd, generator=g)
    flat = x[:rows].view(-1)
    idx = torch.randperm(flat.numel(), generator=g)[:40]
    flat[idx[:8]] = 3.0e4
    flat[idx[8:16]] = -3.0e4
    flat[idx[16:28]] = 1.0e-20
    flat[idx[28:]] = 0.0
    x[0, :hd] = 0.0
    return x.to(torch.bfloat16)


def _gains(hd, seed, wide=False):
    """bf16 [hd] gains: around 1, or (wide) uniform in [-2, 2] with one entry exactly 0"""
    g = torch.Generator().manual_seed(seed)
    gq, gk = ((torch.rand(hd, generator=g) * 4 - 2) if wide else (1 + 0.1 * torch.randn(hd, generator=g)) for _ in range(2))
    if wide:
        gq[5] = 0.0
        gk[hd - 1] = 0.0
    return gq.to(torch.bfloat16), gk.to(torch.bfloat16)


def _pairs(a, w):
    """|a0| + |a1| of every element's rotation pair over columns [0, w)"""
    return np.abs(a[:, :w]).reshape(a.shape[0], -1, 2).sum(-1, keepdims=True).repeat(2, -1).reshape(a.shape[0], w)


def _fwd_tol(y64, n64, w, rotated):
    """Per element.  The result is rounded once to bf16: half a spacing, at most 2^-8 |y|.  Before that, in fp32: the head's sum of
    squares (8 fused steps and log2 G exchange additions, all terms positive: at most 12 roundings, halved by the square root), the
    mean-plus-eps, the rsqrt (1 ulp = 2^-23) and the three products x r, g c and their product -- under 16 roundings of 2^-24
    relative, 2^-20 |n| with n the normalised value.  The rotation then adds, as in test_rotary_gpu._tol, 2^-20 (|n0| + |n1|) over
    the element's pair and carries both inputs' own errors: 2^-19 (|n0| + |n1|) in all."""
    if rotated:
        return 2.0 ** -8 * np.abs(y64[:, :w]) + 2.0 ** -19 * _pairs(n64, w)
    return 2.0 ** -8 * np.abs(y64[:, :w]) + 2.0 ** -20 * np.abs(n64[:, :w])


@pytest.mark.parametrize("keep", [False, True], ids=["nopre", "pre"])
@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("hd", [64, 128])
def test_forward_vs_float64(hd, rows, rotated, keep):
    import dalle_hip as dh
    w, ld = 2 * KH * hd, 3 * KH * hd
    table = _table(hd)
    cs = torch.from_numpy(table).cuda() if rotated else None
    x = _inputs(rows, hd, seed=hd + rows)
    gq, gk = _gains(hd, seed=hd)
    buf = x.clone().cuda()
    pre = torch.full((rows + 1, w), 7.0, dtype=torch.bfloat16).cuda() if keep else None
    dh.qk_norm_fwd(buf, gq.cuda(), gk.cuda(), rows, KS, KH, hd, pre=pre, cs=cs)
    torch.cuda.synchronize()
    y = buf.cpu()
    assert torch.equal(y[:rows, w:].view(torch.int16), x[:rows, w:].view(torch.int16))      # v: bit-identical
    assert torch.equal(y[rows].view(torch.int16), x[rows].view(torch.int16))                # the guard row behind the buffer
    if keep:
        assert torch.equal(pre[:rows].cpu().view(torch.int16), x[:rows, :w].contiguous().view(torch.int16))
        assert bool((pre[rows].float() == 7.0).all())                                       # ... and behind pre
    x64 = x[:rows].double().numpy()
    n64 = qref.qk_norm64(x64, gq.double().numpy(), gk.double().numpy(), KH, hd)
    y64 = qref.qk_norm64(x64, gq.double().numpy(), gk.double().numpy(), KH, hd, KS, table if rotated else None)
    got = y[:rows, :w].double().numpy()
    assert np.isfinite(got).all() and not got[0, :hd].any()                                 # the all-zero head: zeros, not NaN
    err, tol = np.abs(got - y64[:, :w]), _fwd_tol(y64, n64, w, rotated)
    print(f"qk_norm_fwd hd {hd} rows {rows} rope {rotated} pre {keep}: worst err / tol {float((err / np.maximum(tol, 1e-300)).max()):.3f}", flush=True)
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    assert not np.array_equal(got, x64[:, :w])


def _bwd_case(hd, rows, rotated, seed):
    """(x, dy, gains, table | None) and the float64 results; the gains lie in [-2, 2], one entry of each exactly 0"""
    x = _inputs(rows, hd, seed=seed)
    dy = _inputs(rows, hd, seed=seed + 1000)
    dy[0, :hd] = torch.randn(hd, generator=torch.Generator().manual_seed(seed + 2000)).to(torch.bfloat16)   # into the all-zero head
    gq, gk = _gains(hd, seed=seed, wide=True)
    table = _table(hd) if rotated else None
    ref = qref.qk_norm_bwd64(dy[:rows].double().numpy(), x[:rows].double().numpy(), gq.double().numpy(), gk.double().numpy(), KH, hd, KS, table)
    return x, dy, gq, gk, table, ref


def _run_bwd(x, dy, gq, gk, table, rows, hd):
    import dalle_hip as dh
    w = 2 * KH * hd
    buf = dy.clone().cuda()
    pre = x[:, :w].contiguous().cuda()
    dg = torch.full((2, hd + 4), 5.0, dtype=torch.float32).cuda()      # written, not accumulated; four guard floats behind each
    ws = torch.empty(dh.qk_norm_bwd_workspace_bytes(rows, hd), dtype=torch.uint8).cuda()
    dh.qk_norm_bwd(buf, pre, gq.cuda(), gk.cuda(), dg[0], dg[1], ws, rows, KS, KH, hd, cs=None if table is None else torch.from_numpy(table).cuda())
    torch.cuda.synchronize()
    assert bool((dg[:, hd:] == 5.0).all())
    return buf.cpu(), dg[:, :hd].cpu()


@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("hd", [64, 128])
def test_backward_vs_float64(hd, rows, rotated):
    """dx per element.  With D_j = |dy_j| (rotated back, in fp32: |dy0| + |dy1| over the pair, three roundings of it), A_j = |u_j| D_j
    and Mbar = mean_j(A_j |xh_j|): a = u dy carries the rounding of g c, the product's and dy's three, under 2^-21 A_j; xh two (r is
    the float64 value rounded, then the product); the mean m = mean_j(a_j xh_j) under 16 (products, 8 fused steps, log2 G exchange
    additions, the division) plus its operands' seven; a - xh m adds the product's and the difference's, the factor r two more
    relative to the result.  Absolute: r [2^-21 A_j + |xh_j| Mbar (2^-20 + 2^-21)] + 2^-22 |dx|, under
    2^-19 r (A_j + |xh_j| Mbar) + 2^-22 |dx|; the result is then rounded once to bf16, 2^-8 |dx|.
    dgq, dgk: |error| <= n 2^-24 sum |terms| with n = rows, the number of summed rows (the kernel sums float64 terms in float64 and
    rounds once).  Two runs give equal bits.  v and the guard row stay bit-identical."""
    w = 2 * KH * hd
    x, dy, gq, gk, table, (dx64, dgq64, dgk64, dyu, mag) = _bwd_case(hd, rows, rotated, seed=3 * hd + rows)
    got, dg = _run_bwd(x, dy, gq, gk, table, rows, hd)
    again, dg2 = _run_bwd(x, dy, gq, gk, table, rows, hd)
    assert torch.equal(got.view(torch.int16), again.view(torch.int16)) and torch.equal(dg.view(torch.int32), dg2.view(torch.int32))
    assert torch.equal(got[:rows, w:].view(torch.int16), dy[:rows, w:].view(torch.int16))
    assert torch.equal(got[rows].view(torch.int16), dy[rows].view(torch.int16))
    x64 = x[:rows, :w].double().numpy().reshape(rows, 2, KH, hd)
    r = 1.0 / np.sqrt((x64 ** 2).mean(-1, keepdims=True) + qref.EPS)
    xh = np.abs(x64 * r)
    u = np.stack([gq.double().numpy() * hd ** -0.5, gk.double().numpy()]).reshape(2, 1, hd)
    # (the pair of the RAW dy: the rotation's error scales with its inputs, and |rotated dy_j| <= |dy0| + |dy1|)
    D = (_pairs(dy[:rows].double().numpy(), w) if rotated else np.abs(dyu[:, :w])).reshape(rows, 2, KH, hd)
    Aj = np.abs(u) * D
    model = (r * (Aj + xh * (Aj * xh).mean(-1, keepdims=True))).reshape(rows, w)
    tol = (2.0 ** -8 + 2.0 ** -22) * np.abs(dx64[:, :w]) + 2.0 ** -19 * model
    g = got[:rows, :w].double().numpy()
    assert np.isfinite(g).all()
    err = np.abs(g - dx64[:, :w])
    print(f"qk_norm_bwd hd {hd} rows {rows} rope {rotated}: dx worst err / tol {float((err / np.maximum(tol, 1e-300)).max()):.3f}", flush=True)
    assert (err <= tol).all(), float((err / np.maximum(tol, 1e-300)).max())
    assert float(np.abs(dx64[0, :hd]).max()) > 0 and float(np.abs(g[0, :hd]).max()) > 0     # the all-zero head passes r u dy on
    for name, have, want, m in (("dgq", dg[0], dgq64, mag[0]), ("dgk", dg[1], dgk64, mag[1])):
        e, bound = np.abs(have.double().numpy() - want), rows * 2.0 ** -24 * m
        print(f"    {name}: worst err / bound {float((e / np.maximum(bound, 1e-300)).max()):.3f}", flush=True)
        assert (e <= bound).all(), (name, float((e / np.maximum(bound, 1e-300)).max()))
        assert float(np.abs(want).max()) > 0


@pytest.mark.parametrize("rotated", [False, True], ids=["plain", "rope"])
@pytest.mark.parametrize("hd", [64, 128])
def test_decode_equals_the_rows_of_the_full_kernel(hd, rotated):
    import dalle_hip as dh
    B, ld = 3, 3 * KH * hd
    cs = torch.from_numpy(_table(hd, "1d")).cuda() if rotated else None
    gq, gk = (t.cuda() for t in _gains(hd, seed=hd + 1))
    g = torch.Generator().manual_seed(hd)
    fresh = torch.randn(B, ld, generator=g).to(torch.bfloat16).cuda()
    guard = torch.randn(B + 1, ld, generator=g).to(torch.bfloat16).cuda()      # decode buffers with a guard row
    pos_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    for pos, by_dev in ((0, False), (17, False), (KS - 1, False), (0, True), (17, True), (KS - 1, True)):
        full = torch.zeros(B * KS, ld, dtype=torch.bfloat16, device="cuda")
        full[pos::KS] = fresh
        dh.qk_norm_fwd(full, gq, gk, B * KS, KS, KH, hd, cs=cs)
        buf = guard.clone()
        buf[:B] = fresh
        if by_dev:
            pos_dev.fill_(pos)
            dh.qk_norm_decode(buf, gq, gk, B, KS, KH, hd, cs=cs, pos=12345, pos_dev=pos_dev)      # the by-value position is ignored
        else:
            dh.qk_norm_decode(buf, gq, gk, B, KS, KH, hd, cs=cs, pos=pos)
        torch.cuda.synchronize()
        assert torch.equal(buf[:B].view(torch.int16), full[pos::KS].view(torch.int16)), (pos, by_dev)
        assert torch.equal(buf[B].view(torch.int16), guard[B].view(torch.int16))
        assert not torch.equal(buf[:B], fresh)
    for bad in (KS, -1):
        pos_dev.fill_(bad)
        buf = fresh.clone()
        dh.qk_norm_decode(buf, gq, gk, B, KS, KH, hd, cs=cs, pos_dev=pos_dev)
        torch.cuda.synchronize()
        if rotated:      # with a table an out-of-range device position makes the launch a no-op; without one it is not read
            assert torch.equal(buf.view(torch.int16), fresh.view(torch.int16)), bad
        else:
            assert torch.equal(buf[:, 2 * KH * hd:].view(torch.int16), fresh[:, 2 * KH * hd:].view(torch.int16))


# ------------------------------------------------------------------ engine
GAIN_SEED = 5


def _setup(width=256, heads=2, qk=True, hparams=None, seed=0, batch=2):
    """(cfg, model, P, tokens) on engine_case's inputs: P = the oracle's weights plus, with the key on, the perturbed gains"""
    return build(width, heads, batch=batch, seed=seed, hparams=dict(qk_norm=qk, **(hparams or {})),
                 weights=(lambda P0, cfg: qref.with_gains(P0, cfg, seed=GAIN_SEED)) if qk is True else None)


@pytest.mark.parametrize("width,scheme,patterns", [(256, None, None), (128, "1d", None), (256, "axial", PATTERNS)],
                         ids=["hd128", "hd64-1d", "hd128-axial-masked"])
def test_engine_step_vs_qk_norm_fp32_oracle(width, scheme, patterns):
    """the project's bounds of tests/parity.py check_report: loss 5e-4 relative, worst gradient tensor 4.8e-2 relative L2, the gains'
    gradients among them (gains 1 + N(0, 0.05), qk_norm_ref.with_gains)"""
    from src.dalle_mtf.masks import layer_masks
    from src.dalle_mtf.rotary import rotary_table
    cfg, model, Pg, tokens = _setup(width, hparams=dict(rotary_emb=scheme or "absent", attention_pattern=patterns or "absent"))
    eng = model.engine
    assert eng.qk_norm is True and eng.qk_pre is not None and tuple(eng.qk_pre[0].shape) == (eng.M, 2 * width)
    assert eng.qk_pre[0].data_ptr() != eng.qk_pre[1].data_ptr() and (eng.rope_cs is not None) == (scheme is not None)
    loss = float(step(eng, tokens)[0].item())
    gh = eng.export_reference(eng.g)
    masks = layer_masks(patterns, cfg.n_layers, T, P) if patterns is not None else None
    table = rotary_table(scheme, T, P, eng.hd) if scheme else None
    loss_o, go = qref.loss_and_grads(Pg, tokens, cfg, table=table, masks=masks)
    assert set(gh) == set(go)
    tab = {k: rel_l2(gh[k], go[k]) for k in go}
    worst = max((e, k) for k, e in tab.items())
    gains = {k: round(e, 5) for k, e in tab.items() if k.endswith(qref.GAINS)}
    print(f"qk_norm n_embd {width} rotary {scheme} masked {patterns is not None}: loss {loss} oracle {loss_o} worst grad {worst}; "
          f"gain tensors {gains}", flush=True)
    assert abs(loss - loss_o) <= 5e-4 * abs(loss_o), (loss, loss_o)
    assert worst[0] <= 4.8e-2, worst


def test_the_normalisation_is_live():
    """attn/q and attn/k scaled by 2 (chosen on the CPU: the normalised model's gradients of these weights then halve, being
    homogeneous of degree -1 in them, and the qk-norm and the key-off fp32 oracles differ by 0.970 .. 0.992 relative L2 on those
    tensors -- at the unscaled weights only by 0.17 .. 0.27; asserted > 0.2 below): the engine's q / k gradients are at least ten
    times nearer the qk-norm oracle than the key-off one"""
    import dalle_step_ref as sref
    cfg, model, Pg, tokens = _setup()
    eng = model.engine
    Pg = {k: (v * np.float32(2.0) if k.endswith(("attn/q", "attn/k")) else v) for k, v in Pg.items()}
    eng.load_reference_params(Pg)
    step(eng, tokens)
    gh = eng.export_reference(eng.g)
    _, g_on = qref.loss_and_grads(Pg, tokens, cfg)
    _, g_off = sref.loss_and_grads({k: v for k, v in Pg.items() if not k.endswith(qref.GAINS)}, tokens, cfg)
    for k in (k for k in g_on if k.endswith(("attn/q", "attn/k"))):
        assert rel_l2(g_on[k], g_off[k]) > 0.2, k
        near, far = rel_l2(gh[k], g_on[k]), rel_l2(gh[k], g_off[k])
        print(f"live {k}: vs qk-norm oracle {near:.4f}, vs key-off oracle {far:.4f}", flush=True)
        assert far >= 10 * near, (k, near, far)


def test_off_is_off():
    """the key absent, None and False: bit-identical loss and flat gradient, the plain layout, no pre buffer, no state-dict entry"""
    from src.dalle_mtf.layout import ParamLayout
    out = []
    for qk in ("absent", None, False):
        _, model, _, tokens = _setup(qk=qk)
        eng = model.engine
        assert eng.qk_norm is False and eng.qk_pre is None and "qk_norm" not in eng.state_dict()
        assert eng.lay.total == ParamLayout(256, 3, 2, eng.V, eng.S).total and eng.p.numel() == eng.lay.total
        assert not any(n.endswith(qref.GAINS) for n in eng.export_reference())
        out.append(step(eng, tokens))
        del model, eng
        torch.cuda.empty_cache()
    for loss, g in out[1:]:
        assert torch.equal(loss, out[0][0]) and torch.equal(g, out[0][1])
    _, model, _, tokens = _setup()         # ... and on is not off
    assert not torch.equal(step(model.engine, tokens)[0], out[0][0])


def test_recompute_grad_is_bit_identical():
    def make(rc):
        _, model, _, tokens = _setup(hparams=dict(recompute_grad=rc, rotary_emb="axial", residual_dropout=0.1))
        assert (model.engine.qk_pre[0].data_ptr() == model.engine.qk_pre[2].data_ptr()) == rc        # one shared buffer under recompute_grad
        return model, tokens
    res = step_pair(make)
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().sum()) > 0


def test_two_microbatches_equal_one_batch():
    """the comparison and bounds of tests/test_dalle_step_gpu.py::test_microbatched_step_equals_full_batch_step: loss 2e-3 relative,
    flat gradient 2e-2 relative L2, parameters 2.5e-3 after the Adam step; the gains' gradients accumulate with the rest"""
    hp = dict(warmup_steps=0)
    _, full, _, tokens = _setup(hparams=hp)
    tok = torch.from_numpy(tokens).cuda()
    loss_full = float(full.engine.train_step(tok))
    g_full, p_full = full.engine.g.clone(), full.engine.p.clone()
    gains_full = {k: v for k, v in full.engine.export_reference(full.engine.g).items() if k.endswith(qref.GAINS)}
    del full
    torch.cuda.empty_cache()
    from src.dalle_mtf.models import DALLE
    cfg, P0, _ = inputs()
    mb = DALLE(n_embd=256, text_vocab_size=TV, image_vocab_size=IV, text_seq_len=T, image_seq_len=P, n_layers=3, n_heads=2, batch_size=1,
               global_batch_size=1, params=dict(HP, qk_norm=True, num_microbatches=2, **hp)).engine
    mb.load_reference_params(qref.with_gains(P0, cfg, seed=GAIN_SEED))
    loss_mb = float(mb.train_step(tok))
    assert mb.global_step == 1
    assert abs(loss_mb - loss_full) <= 2e-3 * abs(loss_full), (loss_mb, loss_full)
    num, den = float((mb.g - g_full).norm()), float(g_full.norm())
    print(f"qk_norm micro-batches: loss {loss_mb} vs {loss_full}, flat gradient rel L2 {num / den:.5f}", flush=True)
    assert num <= 2e-2 * den, (num, den)
    assert float((mb.p - p_full).abs().max()) <= 2.5e-3
    for k, v in mb.export_reference(mb.g).items():
        if k.endswith(qref.GAINS):
            assert float(np.abs(v).max()) > 0 and float(np.abs(gains_full[k]).max()) > 0, k


def test_adafactor_and_ema_move_the_gains():
    _, model, Pg, tokens = _setup(hparams=dict(optimizer="adafactor", ema_decay=0.9))
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    eng.global_step = 5                    # past the warm-up: a learning rate above 0
    losses = [float(eng.train_step(tok).item()) for _ in range(2)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    p, ema, slots = eng.export_reference(eng.p), eng.export_reference(eng.ema), eng.export_adafactor_slots()
    for i in range(3):
        for g in qref.GAINS:
            k = f"layer_{i}/{g}"
            assert p[k].shape == (128,) and not np.array_equal(p[k], Pg[k]), k                    # the optimizer moved it
            assert not np.array_equal(ema[k], Pg[k]) and not np.array_equal(ema[k], p[k]), k      # the average follows behind
            assert slots[k + "_slot_v"].shape == (128,) and k + "_slot_vr" not in slots           # unfactored
    with eng.ema_weights():
        eng.forward(tok, need_grad=False)
        assert torch.isfinite(eng.logits()).all()


def test_decode_logits_and_samplers():
    """decode-step logits (graph and eager) against the full forward at every image position: the existing 3e-2 relative bound;
    graph-replayed, host-launched and unfused-draw samplers give equal tokens; a guided sample equals its decode_graph=False twin"""
    _, model, _, tokens = _setup(hparams=dict(rotary_emb="axial"))
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    for graph in (True, False):
        worst = decode_worst(eng, tok, graph=graph)
        print(f"qk_norm decode (graph={graph}) vs full forward logits: worst relative {worst}", flush=True)
        assert worst <= 3e-2, (graph, worst)
    samplers_agree(eng, tok[:, :T].contiguous())


def test_checkpoint_records_and_checks_the_key():
    _, model, _, tokens = _setup()
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    eng.forward(tok, need_grad=False)
    want = eng.logits().clone()
    sd = eng.state_dict()
    assert sd["qk_norm"] is True and sd["p"].numel() == eng.lay.total
    del model, eng
    _, off, _, _ = _setup(qk="absent")
    with pytest.raises(ValueError, match="qk_norm") as e:
        off.engine.load_state_dict(sd)
    assert "qk_norm on" in str(e.value) and "qk_norm off" in str(e.value), str(e.value)      # names both settings
    sd_off = off.engine.state_dict()
    assert "qk_norm" not in sd_off
    before = off.engine.p.detach().cpu().clone()
    off.engine.load_state_dict(sd_off)                      # a checkpoint without the key loads into an off model
    assert torch.equal(off.engine.p.cpu(), before)
    del off
    torch.cuda.empty_cache()
    _, same, _, _ = _setup(seed=7)                          # other initial weights: the logits below are the checkpoint's
    with pytest.raises(ValueError, match="qk_norm") as e:
        same.engine.load_state_dict(sd_off)                 # ... and not into an on model
    assert "qk_norm on" in str(e.value) and "qk_norm off" in str(e.value), str(e.value)
    same.engine.load_state_dict(sd)
    same.engine.forward(tok, need_grad=False)
    assert torch.equal(same.engine.logits(), want)
