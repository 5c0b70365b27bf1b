"""Head dim 64 on the GPU: the four head-dim-64 attention kernels against fp32 autograd and against the tested head-dim-128 kernels
on zero-padded heads, their edge cases, determinism and the decode contract; then the engine at n_embd / n_heads = 64 against the
oracles (small shapes and the dalle_example dimensions with 8 heads), batch additivity of its gradient and its samplers."""
import numpy as np
import pytest
import torch

import attention_bwd_ref as ab
import attention_fwd_ref as af
import dalle_hip as dh  # noqa: E402  (path set up by conftest)

pytestmark = pytest.mark.gpu
DEV = "cuda"
HD = 64


def _close(got, ref, rtol, atol, what=""):
    got, ref = got.float().cpu(), ref.float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tol; max err {float(err.max()):.4g}"


def _attn_ref(qkv, B, H, S, hd=HD):
    t = qkv.float().view(B, S, 3, H, hd)
    q, k, v = (t[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    logits = (q @ k.transpose(-1, -2)).masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool), 1), float("-inf"))
    o = torch.softmax(logits, -1) @ v
    return o.permute(0, 2, 1, 3).reshape(B * S, H * hd), torch.logsumexp(logits, -1)


def _inputs(B, H, S, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3, H, HD, generator=g)
    qkv[:, 0] *= 0.17          # logits O(1): the reference folds 1/sqrt(k) into Wq's initialiser
    return qkv.view(B * S, 3 * H * HD).to(torch.bfloat16), torch.randn(B * S, H * HD, generator=g).to(torch.bfloat16)


def _run(qkv, d_o, B, H, S, hd=HD, saved=None):
    """forward + backward on the device: (o, lse, dqkv) -- o, lse of this forward; saved = (o, lse): what the backward takes instead"""
    d = H * hd
    qd = qkv.to(DEV)
    o = torch.zeros(B * S, d, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(B, H, S, dtype=torch.float32, device=DEV)
    dh.attention_fwd(qd, o, lse, B, H, S, head_dim=hd)
    bo, blse = (o, lse) if saved is None else (saved[0].to(DEV), saved[1].to(DEV))
    dqkv = torch.zeros(B * S, 3 * d, dtype=torch.bfloat16, device=DEV)
    dh.attention_bwd(qd, bo, d_o.to(DEV), blse, torch.zeros(3, B, H, S, dtype=torch.float32, device=DEV), dqkv, B, H, S, head_dim=hd)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu(), dqkv.cpu()


def _vs_autograd(B, H, S):
    """the tolerances of tests/test_kernels_gpu.py::_attention_fwd_bwd"""
    qkv, d_o = _inputs(B, H, S, seed=S)
    o, lse, dqkv = _run(qkv, d_o, B, H, S)
    qr = qkv.float().requires_grad_(True)
    o_ref, lse_ref = _attn_ref(qr, B, H, S)
    _close(lse, lse_ref.detach(), 2e-3, 2e-3, "lse")
    _close(o, o_ref.detach(), 1.6e-2, 1.5e-2, "o")
    o_ref.backward(d_o.float())
    d = H * HD
    gref, got = qr.grad.view(B * S, 3, d), dqkv.float().view(B * S, 3, d)
    for i, nm in enumerate("qkv"):
        _close(got[:, i], gref[:, i], 3e-2, 2e-2 * float(gref[:, i].abs().max()), f"d{nm}")
    # per-row budget against the float64 spec of the backward on the kernel's own saved forward (tests/attention_bwd_ref.py)
    ab.within_budget(dqkv, ab.make_inputs(qkv, o, lse, d_o, B, H, S, HD), label=f"_vs_autograd {(B, H, S)}")
    # ... and the forward's own budget on that o and lse (tests/attention_fwd_ref.py)
    af.within_budget_fwd(o, lse, af.make_inputs(qkv, B, H, S, HD), label=f"_vs_autograd forward {(B, H, S)}")
    return o, lse, dqkv


@pytest.mark.parametrize("xcd", [8, 0])
@pytest.mark.parametrize("B,H,S", [(1, 1, 128), (2, 2, 272), (1, 2, 384), (1, 1, 72), (3, 1, 384), (5, 2, 200),
                                   (2, 1, 40), (1, 1, 8), (1, 2, 520), (1, 1, 1280)])
def test_attention64_vs_fp32_autograd(B, H, S, xcd):
    dh.set_option("attn_xcd", xcd)
    try:
        _vs_autograd(B, H, S)
    finally:
        dh.set_option("attn_xcd", 8)


@pytest.mark.parametrize("xcd", [8, 0])
@pytest.mark.parametrize("B,H,S", [(4, 2, 272), (8, 16, 1152)])
def test_attention64_persistent_schedules(B, H, S, xcd):
    """(8, 16, 1152): 1152 items, several per persistent block of every kernel"""
    dh.set_option("attn_xcd", xcd)
    try:
        _vs_autograd(B, H, S)
    finally:
        dh.set_option("attn_xcd", 8)


@pytest.mark.parametrize("B,H,S", [(2, 2, 272), (1, 4, 1280), (2, 1, 72), (8, 8, 1152)])
def test_attention64_equals_zero_padded_128_kernels(B, H, S):
    """Each 64-wide head embedded in a 128-wide head with zeros: scores, softmax and the unpadded columns of o / dq / dk / dv are
    the same mathematics, so the tested 128 kernels are a reference on the SAME bf16 inputs.  o: the 128 forward rounds P at a
    power-of-two scale of its integer running maximum and normalises by the rounded sum, this one at the exact maximum -- one bf16
    ulp of the output range; lse: fp32 summation order.  Both backwards take the SAME saved forward (the 64 kernel's o, zero-padded,
    and lse): with each its own o, the o rounding difference enters every dS of a row through delta = rowsum(dO * o) and moved 0.01 -
    0.2 % of the dq elements by one bf16 ulp.  Gradients: bf16 rounding of the outputs (relative 2^-8) plus accumulation-order noise
    of values near zero."""
    qkv, d_o = _inputs(B, H, S, seed=S + 7)
    o, lse, dqkv = _run(qkv, d_o, B, H, S)
    pad = torch.zeros(B * S, 3, H, 128, dtype=torch.bfloat16)
    pad[..., :HD] = qkv.view(B * S, 3, H, HD)
    dpad = torch.zeros(B * S, H, 128, dtype=torch.bfloat16)
    dpad[..., :HD] = d_o.view(B * S, H, HD)
    opad = torch.zeros(B * S, H, 128, dtype=torch.bfloat16)
    opad[..., :HD] = o.view(B * S, H, HD)
    o1, lse1, dqkv1 = _run(pad.view(B * S, -1), dpad.view(B * S, -1), B, H, S, hd=128, saved=(opad.view(B * S, -1), lse))
    o1 = o1.view(B * S, H, 128)[..., :HD].reshape(B * S, H * HD)
    dqkv1 = dqkv1.view(B * S, 3, H, 128)[..., :HD].reshape(B * S, 3 * H * HD)
    assert float((o.float() - o1.float()).abs().max()) <= 2.0 ** -7 * float(o1.float().abs().max())
    assert float((lse - lse1).abs().max()) <= 1e-5, float((lse - lse1).abs().max())
    g, g1 = dqkv.float().view(B * S, 3, -1), dqkv1.float().view(B * S, 3, -1)
    for i, nm in enumerate("qkv"):
        _close(g[:, i], g1[:, i], 2.0 ** -7, 1e-3 * float(g1[:, i].abs().max()), f"d{nm} vs padded 128 kernels")


@pytest.mark.parametrize("keyrow,qrow,mult", [(700, 900, 3.0), (5, 70, 2.0), (643, 900, 3.0), (675, 901, 1.5), (130, 140, 3.0), (1279, 1279, 3.0)])
def test_attention64_fwd_late_spike(keyrow, qrow, mult):
    """one key far above everything a query has seen before, in the first tile, a steady-state tile and on the diagonal, in lower
    and upper half-row lanes: the rescale must fire and the row maximum must cover both half rows"""
    B, H, S = 1, 1, 1280
    torch.manual_seed(5)
    qkv = torch.randn(S, 3 * HD).to(torch.bfloat16)
    qkv[keyrow, HD:2 * HD] = (qkv[qrow, :HD].float() * mult).to(torch.bfloat16)
    o = torch.zeros(S, HD, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(1, 1, S, dtype=torch.float32, device=DEV)
    dh.attention_fwd(qkv.to(DEV), o, lse, B, H, S, head_dim=HD)
    o_ref, lse_ref = _attn_ref(qkv, B, H, S)
    assert torch.isfinite(lse).all() and torch.isfinite(o.float()).all()
    _close(lse, lse_ref, 1e-5, 2e-3, "lse with a late spike")
    _close(o, o_ref, 1.6e-2, 3e-2, "o with a late spike")


def test_attention64_row0_kat():
    """causal mask: query 0 attends only to key 0 -> o[0] == v[0] exactly"""
    S = 128
    qkv = (torch.randn(S, 3 * HD, generator=torch.Generator().manual_seed(11))).to(torch.bfloat16).to(DEV)
    o = torch.zeros(S, HD, dtype=torch.bfloat16, device=DEV)
    lse = torch.zeros(1, 1, S, dtype=torch.float32, device=DEV)
    dh.attention_fwd(qkv, o, lse, 1, 1, S, head_dim=HD)
    assert torch.equal(o[0].cpu(), qkv[0, 2 * HD:].cpu())


def test_attention64_deterministic_and_reserved_cus():
    """no atomics, fixed reduction orders: two runs give the same bits, and so does the persistent grid with 16 CUs left free"""
    B, H, S = 8, 4, 640
    qkv, d_o = _inputs(B, H, S, seed=3)
    a = _run(qkv, d_o, B, H, S)
    b = _run(qkv, d_o, B, H, S)
    dh.set_option("reserve_cus", 16)
    try:
        c = _run(qkv, d_o, B, H, S)
    finally:
        dh.set_option("reserve_cus", 0)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("B,H,S", [(2, 1, 72), (3, 2, 320)])
def test_attention64_decode_vs_fp32_math(B, H, S):
    """positions at the start, at 64-key chunk boundaries and at the end, vs fp32 softmax(q K^T) V; the graph-replayable form
    (pos_dev, fresh) gives the same bits and moves the staging row into the cache"""
    d = H * HD
    qkv = (torch.randn(B * S, 3 * d, generator=torch.Generator().manual_seed(S)) * 0.4).to(torch.bfloat16)
    qd = qkv.cuda()
    o = torch.empty(B, d, dtype=torch.bfloat16, device=DEV)
    f = qkv.float().view(B, S, 3, H, HD)
    for pos in sorted({0, 1, 63, 64, 65, 127, 128, S // 2, S - 2, S - 1} & set(range(S))):
        dh.attention_decode(qd, o, B, H, S, pos, head_dim=HD)
        q, k, v = f[:, pos, 0], f[:, :pos + 1, 1], f[:, :pos + 1, 2]
        w = torch.softmax(torch.einsum("bhd,bkhd->bhk", q, k), -1)
        ref = torch.einsum("bhk,bkhd->bhd", w, v).reshape(B, d)
        err = float((o.float().cpu() - ref).abs().max())
        assert err <= 1.6e-2 * float(ref.abs().max()) + 2e-3, (pos, err)
        cache = qd.clone()
        cache.view(B, S, 3 * d)[:, pos] = 0
        fresh = qd.view(B, S, 3 * d)[:, pos].contiguous()
        o2 = torch.full_like(o, 7.0)
        dh.attention_decode(cache, o2, B, H, S, 0, fresh=fresh, pos_dev=torch.tensor([pos], dtype=torch.int32, device=DEV), head_dim=HD)
        assert torch.equal(o2, o), pos
        assert torch.equal(cache, qd), pos
    o2.fill_(7.0)
    dh.attention_decode(cache, o2, B, H, S, 0, fresh=fresh, pos_dev=torch.tensor([S], dtype=torch.int32, device=DEV), head_dim=HD)
    torch.cuda.synchronize()
    assert bool((o2 == 7.0).all()) and torch.equal(cache, qd)


# ------------------------------------------------------------------ the engine at n_embd / n_heads = 64

@pytest.mark.parametrize("n_embd,n_heads", [(128, 2), (256, 4)])
def test_engine_step_head_dim64_vs_oracle(n_embd, n_heads):
    from parity import check_report, compare_step
    rep = compare_step(n_embd=n_embd, n_heads=n_heads, T=16, P=256)
    check_report(rep)


def test_dalle_example_dimensions_with_8_heads_vs_oracles():
    """n_embd 512, 8 heads (head dim 64), 6 layers, 256 + 1024 positions, B = 2: the bounds of
    tests/test_headline_parity_gpu.py::test_dalle_example_shape_step_vs_fp32_oracle (fp32 oracle: loss 2e-4, worst tensor 0.042,
    grad norm 2e-3; bf16 oracle; teacher-forced oracle with the flash-style delta) -- the attention arithmetic is the same per score,
    only the contraction length of q.k and of the products through d halves, so none of the error terms grows."""
    from parity import check_report, compare_step
    from test_headline_parity_gpu import BF16_ORACLE_GRAD_TOL, DALLE_EXAMPLE, FORCED_FA_ORACLE_GRAD_TOL
    rep = compare_step(B=2, seed=21, steps=1, perturb=0.02, bf16_oracle=True, per_tensor=True, bf16_grad_oracle=True,
                       **dict(DALLE_EXAMPLE, n_heads=8))
    check_report(rep, loss_rtol=2e-4, grad_tol=0.042, gn_rtol=2e-3)
    s0 = rep["steps"][0]
    print("worst vs fp32:", s0["worst_grad_rel_l2_vs_fp32_oracle"], "vs bf16:", s0["worst_grad_rel_l2_vs_bf16_oracle"],
          "forced fa:", s0["worst_grad_rel_l2_vs_forced_fp32w_fa_oracle"], flush=True)
    assert abs(s0["loss_hip"] - s0["loss_oracle_bf16"]) <= 2e-4 * abs(s0["loss_oracle_bf16"]), s0
    assert s0["worst_grad_rel_l2_vs_bf16_oracle"][0] <= BF16_ORACLE_GRAD_TOL, s0["worst_grad_rel_l2_vs_bf16_oracle"]
    assert s0["worst_grad_rel_l2_vs_forced_fp32w_fa_oracle"][0] <= FORCED_FA_ORACLE_GRAD_TOL, s0["worst_grad_rel_l2_vs_forced_fp32w_fa_oracle"]


def _engine8(B):
    from src.dalle_mtf.engine import DalleEngine
    eng = DalleEngine(512, 6, 8, 50258, 512, 256, 1024, batch_size=B, global_batch_size=32,
                      hparams=dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0))
    eng.init_params(seed=1234)
    eng.global_step = 1500
    return eng


def test_head_dim64_batch_gradient_equals_the_sum_of_two_sequence_gradients():
    """n_heads = 8 at the benchmark batch: the B = 32 gradient is the sum of the sixteen B = 2 gradients (the bound of
    tests/test_headline_parity_gpu.py: 5e-3 worst tensor, 1e-3 on the head)"""
    from oracle import dalle_oracle as do
    B = 32
    tokens = torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, 256, 50258, seed=1),
                                                 do.synthetic_image_tokens(B, 1024, 512, seed=2), 50258)).cuda()
    big = _engine8(B)
    big.forward(tokens, need_grad=True)
    big.backward(allreduce=False)
    torch.cuda.synchronize()
    gb = big.export_reference(big.g)
    del big
    torch.cuda.empty_cache()
    small = _engine8(2)
    acc = None
    for i in range(0, B, 2):
        small.forward(tokens[i:i + 2].contiguous(), need_grad=True)
        small.backward(allreduce=False)
        torch.cuda.synchronize()
        gs = small.export_reference(small.g)
        acc = {k: v.astype(np.float64) for k, v in gs.items()} if acc is None else {k: acc[k] + gs[k] for k in acc}
    del small
    torch.cuda.empty_cache()
    worst = max((float(np.linalg.norm(gb[k] - acc[k]) / (np.linalg.norm(acc[k]) + 1e-30)), k) for k in gb)
    head = {k: float(np.linalg.norm(gb[k] - acc[k]) / (np.linalg.norm(acc[k]) + 1e-30)) for k in gb if "to_logits" in k}
    print("n_heads 8: B = 32 gradient vs the sum of sixteen B = 2 gradients: worst", worst, "head", head, flush=True)
    assert worst[0] <= 5e-3, worst
    assert all(v <= 1e-3 for v in head.values()), head


def test_head_dim64_samplers_agree():
    """greedy tokens with 8 heads of 64: graph-replayed decode + draw, host-launched draw, ungraphed decode and the
    one-forward-per-token sampler (kv_cache=False) emit the same tokens (a trained-like peaked head: perturbed init)"""
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    T, P, tv, iv, B = 16, 112, 60, 64, 2
    cfg = do.DalleConfig(512, tv, iv, T, P, 2, 8)
    eng = DalleEngine(512, 2, 8, tv, iv, T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10))
    eng.load_reference_params(do.init_params(cfg, seed=9, perturb=0.05))
    toks = torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, T, tv, seed=1),
                                               do.synthetic_image_tokens(B, P, iv, seed=2), tv)).cuda()
    text = toks[:, :T].contiguous()
    a = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True)
    a2 = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True, fused_sampling=False)
    a3 = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True, decode_graph=False)
    assert torch.equal(a, a2) and torch.equal(a, a3)
    b = eng.sample_image_tokens(text, temperature=0.0, kv_cache=False)
    agree = float((a == b).float().mean())
    print("n_heads 8: cached vs uncached greedy tokens agree on", agree, flush=True)
    # the uncached sampler runs the tiled forward, the cached one the decode kernel: logits equal to bf16 noise, so tokens can differ
    # only at near-ties of a random-initialised model's flat logits (tests/test_model_fns_gpu.py checks that at head dim 128)
    assert int((a != b).any(1).sum()) == 0 or agree >= 0.5, agree


def test_head_dim96_still_refused():
    from src.dalle_mtf.engine import DalleEngine
    with pytest.raises(dh.DalleHipError, match="64 and 128"):
        DalleEngine(384, 2, 4, 60, 64, 16, 112, batch_size=2, hparams=dict(lr=1e-3, train_steps=10))
