"""Gated feed-forward on the GPU (config key "ff_glu", DESIGN.md §4 "Gated feed-forward"): dmi_glu_fwd / dmi_glu_bwd against the
float64 gate of tests/glu_ref.py on the bf16 inputs the kernels read, their guard rows and columns, one case past 2 GiB, and the
engine with the key on: the step against the gated fp32 oracle, the gate's two halves, off, recompute_grad, the decode step, the
samplers and checkpoints."""
import numpy as np
import pytest
import torch

import dalle_hip as dh  # noqa: E402  (path set up by conftest)
import glu_ref
from engine_case import P, PATTERNS, T, build, decode_worst, inputs, step, step_pair
from parity import rel_l2

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS32 = 2.0 ** -24
SENTINEL = 0x4B4B           # bf16 bits of 13303808.0: never the result of a case below
GATES = [0.0, 0.75, -0.75, 5.0, -5.0, 9.5, -9.5, 30.0, -30.0]
LARGE = 2.0 ** 20           # exact in bf16; |large * large * 30| stays far inside fp32 and bf16
SIDES = [0.0, LARGE, -LARGE]


def _bits(t):
    return t.view(torch.int16)


def _ulp_bf16(x):
    """the bf16 unit in the last place at |x| (float64 tensor): 2^(e - 7), e = floor(log2 |x|); the smallest normal's below it
    (as tests/test_activation_gpu.py)"""
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def _guarded(rows, ld, seed):
    """bf16 [rows, ld] of the sentinel"""
    return torch.full((rows, ld), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)


def _inputs(M, Hh, ldpre, lddh, seed):
    """pre [M, ldpre] and dh [M, lddh], seeded normal x 3 in bf16, with every (gate, value, dh) combination of the planted values at
    the first flat positions of the [M, Hh] problem (as many as it has)"""
    g = torch.Generator().manual_seed(seed)
    pre = (torch.randn(M, ldpre, generator=g) * 3).to(torch.bfloat16)
    dhh = (torch.randn(M, lddh, generator=g) * 3).to(torch.bfloat16)
    combos = [(a, b, c) for a in GATES for b in SIDES for c in SIDES]
    for i, (gate, val, d_) in enumerate(combos[:M * Hh]):
        m, j = divmod(i, Hh)
        pre[m, Hh + j], pre[m, j], dhh[m, j] = gate, val, d_
    return pre.to(DEV), dhh.to(DEV)


SHAPES = [(1, 8), (37, 136), (300, 1024)]


@pytest.mark.parametrize("act", ["relu", "gelu"])
@pytest.mark.parametrize("pad", [0, 8, 64])
@pytest.mark.parametrize("M,Hh", SHAPES)
def test_glu_kernels_vs_float64(M, Hh, pad, act):
    """h = bf16(val * act(gate)), dpre = bf16([dh * act(gate) | dh * val * act'(gate)]) on the bf16 inputs the kernels read.  Bound per
    element: one bf16 ulp of the exact result plus the fp32 evaluation term of tests/test_activation_gpu.py for the same device
    functions -- gelu: 1.13 eps32 |factor * gate| (|gelu'| <= 1.13 carries the fp32 rounding of the argument), gelu': 4e-6 |dh * val|
    absolute (exp2 / rcp).  The planted gates need no more: at +-30 sigmoid(2u) is exactly 1 / 0 in fp32 and in float64's tanh; at
    -9.5 the float64 form cancels to 0 while fp32 keeps gate * 2^-110 ~ 7e-33 per unit of the other factor, far inside the
    1.13 eps32 |factor * gate| term.  ReGLU multiplies bf16 values (8-bit significands: every product of two is exact in fp32, and
    the three-factor one is a product with 0 or 1), so its outputs are bit-equal to the bf16 rounding of the float64 result.  Rows
    past M, the padding of every row and, for h, nothing else may change: the buffers start as a sentinel."""
    ldpre, ldh, lddh, lddpre = 2 * Hh + pad, Hh + pad, Hh + (8 if pad else 0), 2 * Hh + pad
    pre, dhh = _inputs(M, Hh, ldpre, lddh, seed=M + Hh + pad)
    h = _guarded(M + 2, ldh, 1)
    dpre = _guarded(M + 2, lddpre, 2)
    dh.glu_fwd(pre, ldpre, h, ldh, M, Hh, act)
    dh.glu_bwd(dhh, lddh, pre, ldpre, dpre, lddpre, M, Hh, act)
    torch.cuda.synchronize()
    # guards
    assert (_bits(h[M:]) == SENTINEL).all() and (_bits(h[:M, Hh:]) == SENTINEL).all()
    assert (_bits(dpre[M:]) == SENTINEL).all() and (_bits(dpre[:M, 2 * Hh:]) == SENTINEL).all()
    p64, d64 = pre[:, :2 * Hh].double().cpu(), dhh[:, :Hh].double().cpu()
    val, gate = p64[:, :Hh], p64[:, Hh:]
    ref_h = glu_ref.glu(p64, act)
    ref_d = glu_ref.glu_grad(d64, p64, act)
    got_h, got_d = h[:M, :Hh].cpu(), dpre[:M, :2 * Hh].cpu()
    assert torch.isfinite(got_h.float()).all() and torch.isfinite(got_d.float()).all()
    if act == "relu":
        assert torch.equal(_bits(got_h), _bits(ref_h.to(torch.bfloat16)))
        assert torch.equal(_bits(got_d), _bits(ref_d.to(torch.bfloat16)))
        assert (got_d[:, Hh:][gate <= 0] == 0).all()                  # relu'(0) = 0
        return
    tol_h = _ulp_bf16(ref_h) + 1.13 * EPS32 * (val * gate).abs()
    tol_v = _ulp_bf16(ref_d[:, :Hh]) + 1.13 * EPS32 * (d64 * gate).abs()
    tol_g = _ulp_bf16(ref_d[:, Hh:]) + 4e-6 * (d64 * val).abs()
    for name, got, ref, tol in (("h", got_h, ref_h, tol_h), ("dvalue", got_d[:, :Hh], ref_d[:, :Hh], tol_v),
                                ("dgate", got_d[:, Hh:], ref_d[:, Hh:], tol_g)):
        err = (got.double() - ref).abs()
        worst = float((err / tol).max())
        print(f"glu {act} M {M} Hh {Hh} pad {pad} {name}: worst error / bound {worst:.3f}", flush=True)
        assert (err <= tol).all(), (name, worst, int((err > tol).sum()))
    # the saturated gates are reproduced exactly: gate 30 -> sigmoid(2u) = 1, h = 30 value and dgate = dh value; gate -30 -> zeros
    sat, cut = gate == 30.0, gate == -30.0
    if sat.any():
        assert torch.equal(_bits(got_h[sat]), _bits((30.0 * val[sat]).to(torch.bfloat16)))
        assert torch.equal(_bits(got_d[:, Hh:][sat]), _bits((d64 * val)[sat].to(torch.bfloat16)))
        assert (got_h[cut] == 0).all() and (got_d[:, :Hh][cut] == 0).all() and (got_d[:, Hh:][cut] == 0).all()


def test_glu_kernels_past_two_gib():
    """M = 270 000 rows of Hh = 2048 at ldpre = 4104: pre and dpre are 2.2 GB each, and row 261 636 straddles byte offset 2^31.
    That row with its neighbours and the last 64 rows against float64 (the GEGLU bounds above); one allocation, no loop over sizes."""
    M, Hh, ld = 270000, 2048, 4104
    row = 2 ** 31 // (ld * 2)
    assert row * ld * 2 < 2 ** 31 < (row + 1) * ld * 2 and M * ld * 2 > 2.2e9
    gen = torch.Generator(device=DEV).manual_seed(7)
    pre = torch.empty(M, ld, dtype=torch.bfloat16, device=DEV).normal_(0, 3, generator=gen)
    dhh = torch.empty(M, Hh, dtype=torch.bfloat16, device=DEV).normal_(0, 3, generator=gen)
    h = torch.empty(M, Hh, dtype=torch.bfloat16, device=DEV)
    dpre = torch.empty(M, ld, dtype=torch.bfloat16, device=DEV)
    _bits(h).fill_(SENTINEL)
    _bits(dpre).fill_(SENTINEL)
    dh.glu_fwd(pre, ld, h, Hh, M, Hh, "gelu")
    dh.glu_bwd(dhh, Hh, pre, ld, dpre, ld, M, Hh, "gelu")
    torch.cuda.synchronize()
    rows = torch.tensor(list(range(row - 1, row + 2)) + list(range(M - 64, M)), device=DEV)
    p64, d64 = pre[rows, :2 * Hh].double().cpu(), dhh[rows].double().cpu()
    val, gate = p64[:, :Hh], p64[:, Hh:]
    ref_h, ref_d = glu_ref.glu(p64, "gelu"), glu_ref.glu_grad(d64, p64, "gelu")
    got_h, got_d = h[rows].double().cpu(), dpre[rows, :2 * Hh].double().cpu()
    assert ((got_h - ref_h).abs() <= _ulp_bf16(ref_h) + 1.13 * EPS32 * (val * gate).abs()).all()
    assert ((got_d[:, :Hh] - ref_d[:, :Hh]).abs() <= _ulp_bf16(ref_d[:, :Hh]) + 1.13 * EPS32 * (d64 * gate).abs()).all()
    assert ((got_d[:, Hh:] - ref_d[:, Hh:]).abs() <= _ulp_bf16(ref_d[:, Hh:]) + 4e-6 * (d64 * val).abs()).all()
    assert (_bits(dpre[rows, 2 * Hh:]) == SENTINEL).all()       # the padding of the checked rows
    assert float(ref_h.abs().max()) > 1 and float(ref_d.abs().max()) > 1


def test_wrappers_refuse_before_a_launch():
    pre = torch.zeros(4, 128, dtype=torch.bfloat16, device=DEV)
    h = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(dh.DalleHipError, match="ldh"):
        dh.glu_fwd(pre, 128, h, 60, 4, 64, "relu")
    with pytest.raises(dh.DalleHipError, match="aligned"):
        dh.glu_fwd(pre.data_ptr() + 2, 128, h.data_ptr(), 64, 3, 64, "relu")
    with pytest.raises(dh.DalleHipError, match="'relu' or 'gelu'"):
        dh.glu_fwd(pre, 128, h, 64, 4, 64, "silu")
    with pytest.raises(dh.DalleHipError, match="Hh % 8"):
        dh.glu_bwd(h, 64, pre, 128, pre.clone(), 128, 4, 60, "gelu")


# ------------------------------------------------------------------ the engine
def _build(act="gelu", width=256, heads=2, layers=3, glu=True, seed=0, hparams=None, widen_seed=5):
    """(cfg, model, P, tokens): tests/engine_case.py's small case with mlp_linear_1 widened (glu) and loaded"""
    return build(width, heads, layers, seed=seed, hparams=dict(activation_fn=act, ff_glu=glu, **(hparams or {})),
                 weights=(lambda P0, cfg: glu_ref.widen(P0, cfg, seed=widen_seed)) if glu else None)


_ORACLE = {}


def _oracle(act, width, heads, layers=3):
    """the gated fp32 oracle's (loss, gradients) on the default case: computed once per arm, shared, never modified"""
    key = (act, width, heads, layers)
    if key not in _ORACLE:
        cfg, P0, tokens = inputs(width, heads, layers)
        _ORACLE[key] = glu_ref.loss_and_grads(glu_ref.widen(P0, cfg, seed=5), tokens, cfg, activation=act)
    return _ORACLE[key]


def _check_step(tag, eng, tokens, loss_o, go):
    """tests/parity.py check_report's first-step bounds, the ones of the GELU engine test of the same shapes: loss 5e-4 relative,
    every gradient tensor 4.8e-2 relative L2, the global gradient norm 2e-3 relative"""
    loss = float(step(eng, tokens)[0].item())
    gh = eng.export_reference(eng.g)
    assert set(gh) == set(go)
    table = {k: rel_l2(gh[k], go[k]) for k in go}
    worst = max((e, k) for k, e in table.items())
    ffn = {sfx: round(max(e for n, e in table.items() if n.endswith(sfx)), 5)
           for sfx in ("mlp_linear_1/kernel", "mlp_linear_1/bias", "mlp_linear_2/kernel", "mlp_linear_2/bias")}
    gn_h = float(np.sqrt(sum(float((gh[k].astype(np.float64) ** 2).sum()) for k in gh)))
    gn_o = float(np.sqrt(sum(float((go[k].astype(np.float64) ** 2).sum()) for k in go)))
    print(f"ff_glu {tag}: loss {loss} oracle {loss_o}; worst gradient {worst}; FFN tensors (worst layer) {ffn}; "
          f"grad norm {gn_h} oracle {gn_o}", flush=True)
    assert abs(loss - loss_o) <= 5e-4 * abs(loss_o), (loss, loss_o)
    assert worst[0] <= 4.8e-2, worst
    assert abs(gn_h - gn_o) <= 2e-3 * gn_o, (gn_h, gn_o)


@pytest.mark.parametrize("recompute", [False, True], ids=["stored", "recompute"])
@pytest.mark.parametrize("width,heads", [(256, 2), (128, 2)], ids=["hd128", "hd64"])
@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_engine_step_vs_gated_fp32_oracle(act, width, heads, recompute):
    _, model, _, tokens = _build(act, width, heads, hparams=dict(recompute_grad=recompute))
    eng = model.engine
    assert eng.ff_glu is True and eng.ffn_form == "glu" and eng.F1 == 8 * width and eng.hbits is None
    assert tuple(eng.hpre[0].shape) == (eng.M, 8 * width) and tuple(eng.dpre.shape) == (eng.M, 8 * width)
    assert (eng.hpre[0].data_ptr() == eng.hpre[2].data_ptr()) == recompute
    _check_step(f"{act} n_embd {width} recompute {recompute}", eng, tokens, *_oracle(act, width, heads))


def test_engine_step_n_embd_512_on_the_fused_layernorm_forms():
    """n_embd = 512: the library's predicates answer yes at the gated shapes, so FFN-1's input gradient runs fused with norm_2's
    backward at K = 8d = 4096 and the weight gradients take the plan asked with (d, 8d)"""
    _, model, _, tokens = _build("gelu", 512, 4, layers=2)
    eng = model.engine
    assert eng.wgrad_shapes[1] == (512, 4096)
    print(f"ff_glu n_embd 512: fuse_ln {eng.fuse_ln} fuse_lnbwd {eng.fuse_lnbwd} lnb_batch {eng.lnb_batch} wgrad_group4 {eng.wgrad_group4}",
          flush=True)
    assert eng.fuse_lnbwd == bool(dh.gemm_nt_ln_auto(eng.M, 512, 4096))
    _check_step("gelu n_embd 512", eng, tokens, *_oracle("gelu", 512, 4, 2))


def test_engine_step_with_every_option_on():
    """attention patterns, axial rotary, token shift and loss weights on top of GEGLU"""
    from src.dalle_mtf.masks import layer_masks
    from src.dalle_mtf.rotary import rotary_table
    cfg, model, Pw, tokens = _build("gelu", hparams=dict(attention_pattern=PATTERNS, rotary_emb="axial", token_shift=True,
                                                         text_loss_weight=1.0, image_loss_weight=7.0))
    eng = model.engine
    assert eng.token_shift and eng.rotary == "axial" and eng.loss_weights is not None and any(p is not None for p in eng.attn_plan)
    loss_o, go = glu_ref.loss_and_grads(Pw, tokens, cfg, activation="gelu", masks=layer_masks(PATTERNS, cfg.n_layers, T, P),
                                        table=rotary_table("axial", T, P, eng.hd), token_shift=True, loss_weights=(1.0, 7.0))
    _check_step("gelu, every option", eng, tokens, loss_o, go)


@pytest.mark.parametrize("half", ["value", "gate"])
def test_both_halves_of_w1_are_live(half):
    """N(0, 1) noise on only the value half, or only the gate half, of one layer's W1.  In the fp32 oracle that half's gradient then
    lies 0.46 (value) / 0.74 (gate) relative L2 from the unperturbed one and the loss moves by -8.7e-3 / +4.9e-4 relative (computed
    on the CPU; W2's small init keeps the loss insensitive to the MLP).  The engine must follow: its gradient of that half is more
    than 0.15 from the unperturbed oracle's and within the step bound of the perturbed one's, its loss changes, and the change
    agrees with the oracle's to 1e-3 of the loss (each loss is within 5e-4 relative of its oracle's); for the value half, whose
    effect is above that noise, with the same sign."""
    cfg, model, Pw, tokens = _build("gelu")
    eng, d = model.engine, 256
    k = "layer_1/mlp/mlp_linear_1/kernel"
    cols = slice(0, 4 * d) if half == "value" else slice(4 * d, 8 * d)
    loss0 = float(step(eng, tokens)[0].item())
    P2 = {n: v.copy() for n, v in Pw.items()}
    P2[k][:, cols] += np.random.default_rng(3).standard_normal((d, 4 * d)).astype(np.float32)
    eng.load_reference_params(P2)
    loss1 = float(step(eng, tokens)[0].item())
    g1 = eng.export_reference(eng.g)[k][:, cols]
    lo0, go0 = _oracle("gelu", 256, 2)
    lo1, go1 = glu_ref.loss_and_grads(P2, tokens, cfg, activation="gelu")
    apart, far, near = rel_l2(go1[k][:, cols], go0[k][:, cols]), rel_l2(g1, go0[k][:, cols]), rel_l2(g1, go1[k][:, cols])
    print(f"live {half}: loss {loss0} -> {loss1} (oracle {lo0} -> {lo1}); oracles apart {apart:.4f}, engine vs unperturbed oracle "
          f"{far:.4f}, vs perturbed oracle {near:.4f}", flush=True)
    assert apart > 0.2 and far > 0.15 and near <= 4.8e-2, (apart, far, near)
    assert loss1 != loss0 and abs((loss1 - loss0) - (lo1 - lo0)) <= 1e-3 * abs(lo0), (loss0, loss1, lo0, lo1)
    if half == "value":
        assert abs(lo1 - lo0) > 2e-3 * abs(lo0) and (loss1 - loss0) * (lo1 - lo0) > 0


def test_off_is_off():
    """the key false and the key absent: the same loss and flat gradient, bit for bit, on the plain FFN's launches"""
    out = []
    for glu in (False, "absent"):
        _, model, _, tokens = build(hparams=dict(activation_fn="gelu", ff_glu=glu))
        eng = model.engine
        assert eng.ff_glu is False and eng.ffn_form == "gelu" and eng.dpre is None and eng.F1 == 4 * 256
        assert "ff_glu" not in eng.state_dict()
        out.append(step(eng, tokens))
        eng._prefill(torch.from_numpy(tokens).cuda())
        eng.decode_step(torch.from_numpy(tokens[:, T - 1].copy()).cuda(), T - 1)
        assert eng._dec["pre"] is None
        del model, eng
        torch.cuda.empty_cache()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    h = [__import__("hashlib").sha256(g.cpu().numpy().tobytes() + l.cpu().numpy().tobytes()).hexdigest() for l, g in out]
    assert h[0] == h[1]
    # the same for the default activation, where the plain arm is one of the two ReLU forms
    _, relu, _, _ = _build("absent", glu=False)
    assert relu.engine.ffn_form in ("relu", "relu_bits")


def test_recompute_grad_is_bit_identical():
    res = step_pair(lambda rc: _build("gelu", hparams=dict(recompute_grad=rc, residual_dropout=0.1, embed_dropout=0.1))[1::2])
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert float(res[0][1].abs().sum()) > 0


@pytest.mark.parametrize("act", ["gelu", "relu"])
def test_decode_logits_against_the_full_forward(act):
    """cached decode logits (graph and eager) at every image position: the 3e-2 relative bound of the token-shift decode test"""
    _, model, _, tokens = _build(act)
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    for graph in (True, False):
        worst = decode_worst(eng, tok, graph=graph)
        print(f"ff_glu {act} decode (graph={graph}) vs full forward logits: worst relative {worst}", flush=True)
        assert worst <= 3e-2, (graph, worst)
    assert tuple(eng._dec["pre"].shape) == (2, 8 * 256)


def test_samplers_agree():
    """greedy tokens: graph-replayed decode + draw, host-launched draw and ungraphed decode are equal; the one-forward-per-token
    sampler agrees up to the near-tie rule of the GELU sampler test (equal, or at least half of the tokens equal once a near-tie
    has sent the two down different continuations); and the gated model does not sample what the plain one samples"""
    _, model, _, tokens = _build("gelu")
    eng = model.engine
    text = torch.from_numpy(tokens).cuda()[:, :T].contiguous()
    a = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True)
    a2 = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True, fused_sampling=False)
    a3 = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True, decode_graph=False)
    assert torch.equal(a, a2) and torch.equal(a, a3)
    b = eng.sample_image_tokens(text, temperature=0.0, kv_cache=False)
    agree = float((a == b).float().mean())
    print("ff_glu: cached vs uncached greedy tokens agree on", agree, flush=True)
    assert int((a != b).any(1).sum()) == 0 or agree >= 0.5, agree
    _, plain, _, _ = _build("gelu", glu=False)
    c = plain.engine.sample_image_tokens(text, temperature=0.0, kv_cache=True)
    assert not torch.equal(a, c)


def test_checkpoint_records_and_checks_the_key():
    _, model, _, tokens = _build("gelu")
    eng = model.engine
    tok = torch.from_numpy(tokens).cuda()
    eng.train_step(tok)
    torch.cuda.synchronize()
    sd = eng.state_dict()
    assert sd["ff_glu"] is True and sd["p"].numel() == eng.lay.total
    want = eng.p.detach().cpu().clone()
    _, same, _, _ = _build("gelu", seed=7)             # other initial weights
    assert not torch.equal(same.engine.p.cpu(), want)
    same.engine.load_state_dict(sd)
    assert torch.equal(same.engine.p.cpu(), want) and torch.equal(same.engine.pb.cpu(), eng.pb.cpu())
    no_key = {k: v for k, v in sd.items() if k != "ff_glu"}          # a checkpoint without the key is a plain model's
    with pytest.raises(ValueError, match="ff_glu"):
        same.engine.load_state_dict(no_key)
    del model, eng, same
    torch.cuda.empty_cache()
    _, off, _, _ = _build("gelu", glu=False)
    with pytest.raises(ValueError, match="ff_glu"):
        off.engine.load_state_dict(sd)
    sd_off = off.engine.state_dict()
    assert "ff_glu" not in sd_off
    before = off.engine.p.detach().cpu().clone()
    off.engine.load_state_dict(sd_off)                               # ... and loads as off
    assert torch.equal(off.engine.p.cpu(), before)


def test_adafactor_ema_and_microbatches_train_the_gated_model():
    """the rest of the step composes: Adafactor over the [d, 8d] variable (factored), the weight average, two micro-batches"""
    cfg, model, Pw, tokens = _build("relu", hparams=dict(optimizer="adafactor", ema_decay=0.9, num_microbatches=2))
    eng = model.engine
    tok = torch.from_numpy(np.concatenate([tokens, tokens[::-1]])).cuda()
    losses = [float(eng.train_step(tok).item()) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    k = "layer_0/mlp/mlp_linear_1/kernel"
    assert eng.export_reference(eng.p)[k].shape == (256, 2048) and not np.array_equal(eng.export_reference(eng.p)[k], Pw[k])
    slots = eng.export_adafactor_slots()
    assert slots[k + "_slot_vr"].shape[0] + slots[k + "_slot_vc"].shape[0] == 256 + 2048
    with eng.ema_weights():
        eng.forward(tok[:2].contiguous(), need_grad=False)
        assert torch.isfinite(eng.logits()).all()
