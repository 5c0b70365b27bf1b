"""Masked attention kernels (head dim 128) on the GPU against fp32 autograd with the dense mask: forward, backward, decode, the
causal plan forced through the masked kernels, and tiles the mask leaves empty are never read (NaN-poisoned keys / values)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))

pytestmark = pytest.mark.gpu

import attention_bwd_ref as ab  # noqa: E402
import attention_fwd_ref as af  # noqa: E402
import dalle_hip as dh  # noqa: E402
from src.dalle_mtf.masks import pattern_mask  # noqa: E402

HD = 128


def _ref(qkv, mask, B, H, S):
    x = qkv.float().view(B, S, 3, H, HD).permute(2, 0, 3, 1, 4)   # [3, B, H, S, HD]
    q, k, v = (t.detach().clone().requires_grad_(True) for t in x)
    s = q @ k.transpose(-1, -2)
    s = s.masked_fill(~mask, float("-inf"))
    o = torch.softmax(s, -1) @ v
    return q, k, v, o, torch.logsumexp(s, -1)


def close(got, ref, rtol, atol, what=""):
    """elementwise |got - ref| <= atol + rtol |ref| (the tolerances of test_kernels_gpu.py)"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tol; max err {float(err.max()):.4g}"


def _qkv(B, H, S, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(B * S, 3 * H * HD, device="cuda", generator=g) * 0.35).bfloat16()


def _run(qkv, plan, B, H, S, d_o):
    o = torch.empty(B * S, H * HD, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B * H * S, dtype=torch.float32, device="cuda")
    dh.attention_fwd_masked(qkv, o, lse, plan, B, H, S)
    scratch = torch.empty(3 * B * H * S, dtype=torch.float32, device="cuda")
    dqkv = torch.full_like(qkv, float("nan"))
    dh.attention_bwd_masked(qkv, o, d_o, lse, scratch, dqkv, plan, B, H, S)
    torch.cuda.synchronize()
    return o, lse, dqkv


def _check(mask_np, B=2, H=2, seed=0, xcd=None, qkv=None):
    S = mask_np.shape[0]
    qkv = _qkv(B, H, S, seed) if qkv is None else qkv
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    d_o = (torch.randn(B * S, H * HD, device="cuda", generator=g) * 0.5).bfloat16()
    plan = dh.AttnMaskPlan(mask_np)
    old = dh.get_option("attn_xcd") if xcd is not None else None
    dh.set_option("attn_mask_force", 1)
    try:
        if xcd is not None:
            dh.set_option("attn_xcd", xcd)
        o, lse, dqkv = _run(qkv, plan, B, H, S, d_o)
    finally:
        dh.set_option("attn_mask_force", 0)
        if old is not None:
            dh.set_option("attn_xcd", old)
    mask = torch.from_numpy(mask_np).cuda()
    q, k, v, oref, lse_ref = _ref(qkv, mask, B, H, S)
    oref.backward(d_o.float().view(B, S, H, HD).permute(0, 2, 1, 3))
    o4 = o.view(B, S, H, HD).permute(0, 2, 1, 3)
    assert torch.isfinite(o).all() and torch.isfinite(lse).all()
    close(lse.view(B, H, S), lse_ref, 2e-3, 2e-3, "masked lse")
    close(o4, oref, 1.6e-2, 1.5e-2, "masked o")
    d = dqkv.view(B, S, 3, H, HD).permute(2, 0, 3, 1, 4)
    for name, got, ref in (("dq", d[0], q.grad), ("dk", d[1], k.grad), ("dv", d[2], v.grad)):
        assert torch.isfinite(got).all(), name
        close(got, ref, 3e-2, 2e-2 * float(ref.abs().max()), "masked " + name)
    # per-row budget against the float64 spec of the backward on the kernel's own saved forward (tests/attention_bwd_ref.py)
    ab.within_budget(dqkv, ab.make_inputs(qkv, o, lse, d_o, B, H, S, HD, mask_np), label=f"masked _check {(B, H, S)}")
    # ... and the forward's own budget on that o and lse (tests/attention_fwd_ref.py)
    af.within_budget_fwd(o, lse, af.make_inputs(qkv, B, H, S, HD, mask_np), label=f"masked _check forward {(B, H, S)}")
    return qkv, d_o, plan, o, lse, dqkv


def _block_mask(S, seed, tile=32):
    rng = np.random.default_rng(seed)
    nb = (S + tile - 1) // tile
    blocks = rng.random((nb, nb)) < 0.5
    m = np.kron(blocks, np.ones((tile, tile), dtype=bool))[:S, :S] | (rng.random((S, S)) < 0.1)
    m &= np.tril(np.ones((S, S), dtype=bool))
    m[np.arange(S), np.arange(S)] = True
    return m


@pytest.mark.parametrize("S,seed", [(256, 0), (272, 1), (520, 2)])
def test_random_masks_match_fp32_autograd(S, seed):
    _check(_block_mask(S, seed), seed=seed)


@pytest.mark.parametrize("pattern", ["causal", "local:40", "row", "column", "conv:3"])
def test_named_patterns_match_fp32_autograd(pattern):
    _check(pattern_mask(pattern, 16, 256), B=2, H=4, seed=3)


@pytest.mark.parametrize("xcd", [0, 8])
def test_both_block_schedules(xcd):
    _check(pattern_mask("row", 256, 1024), B=2, H=4, seed=4, xcd=xcd)


def test_forced_causal_plan_matches_dense_kernels():
    B, H, S = 2, 4, 528
    qkv = _qkv(B, H, S, 5)
    g = torch.Generator(device="cuda").manual_seed(6)   # the d_o _check draws for seed 5
    d_o = (torch.randn(B * S, H * HD, device="cuda", generator=g) * 0.5).bfloat16()
    o = torch.empty(B * S, H * HD, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B * H * S, dtype=torch.float32, device="cuda")
    dh.attention_fwd(qkv, o, lse, B, H, S)
    scratch = torch.empty(3 * B * H * S, dtype=torch.float32, device="cuda")
    dqkv = torch.empty_like(qkv)
    dh.attention_bwd(qkv, o, d_o, lse, scratch, dqkv, B, H, S)
    _, _, _, o2, lse2, dqkv2 = _check(np.tril(np.ones((S, S), dtype=bool)), B=B, H=H, seed=5)
    close(o2, o, 1.6e-2, 1.5e-2, "forced causal o")
    close(dqkv2, dqkv, 3e-2, 2e-2 * float(dqkv.float().abs().max()), "forced causal dqkv")
    assert float((lse2 - lse).abs().max()) < 2e-2


def test_empty_tiles_are_never_read():
    """keys 128..255 are attended to by nobody; their own queries see only the 64 text keys.  NaN K / V there changes nothing
    and their dK / dV are exactly 0."""
    B, H, S = 2, 2, 384
    m = np.tril(np.ones((S, S), dtype=bool))
    m[:, 128:256] = False
    m[128:256, :] = False
    m[128:256, :64] = True
    qkv, d_o, plan, o, lse, dqkv = _check(m, B=B, H=H, seed=6)
    poisoned = qkv.clone().view(B, S, 3, H * HD)
    poisoned[:, 128:256, 1:] = float("nan")
    poisoned = poisoned.view(B * S, -1)
    dh.set_option("attn_mask_force", 1)
    try:
        o2, lse2, dqkv2 = _run(poisoned, plan, B, H, S, d_o)
    finally:
        dh.set_option("attn_mask_force", 0)
    assert torch.equal(o2, o) and torch.equal(lse2, lse)
    d2 = dqkv2.view(B, S, 3, H * HD)
    assert torch.equal(d2[:, :, 0], dqkv.view(B, S, 3, H * HD)[:, :, 0])
    assert (d2[:, 128:256, 1:] == 0).all()


@pytest.mark.parametrize("keyrow,qrow,mult", [(700, 900, 3.0), (5, 70, 2.0), (643, 900, 3.0), (1279, 1279, 3.0)])
def test_late_spike(keyrow, qrow, mult):
    """one key far above everything query qrow saw before, on the masked path (row pattern, every key in play is allowed for
    qrow): the rescale must fire and lse / o stay finite and match"""
    B, H, T, P = 1, 1, 256, 1024
    m = pattern_mask("local:1279", T, P)
    m[qrow, :] = np.arange(T + P) <= qrow        # the spiked query sees every key up to itself, the spike included
    m[qrow, 300:310] = False                     # ... but with a hole, so its tiles are partial
    g = torch.Generator().manual_seed(5)
    qkv = torch.randn(T + P, 3 * HD, generator=g).to(torch.bfloat16)
    qkv[keyrow, HD:2 * HD] = (qkv[qrow, :HD].float() * mult).to(torch.bfloat16)
    if keyrow in range(300, 310):
        m[qrow, keyrow] = True
    _check(m, B=B, H=H, qkv=qkv.cuda())


def test_row_zero_is_v0_exactly():
    """query 0 attends only to key 0 under every mask: o[0] == v[0] bit for bit on the masked path"""
    B, H, S = 1, 1, 272
    m = pattern_mask("row", 16, 256)
    plan = dh.AttnMaskPlan(m)
    qkv = _qkv(B, H, S, 11)
    o = torch.zeros(S, HD, dtype=torch.bfloat16, device="cuda")
    lse = torch.zeros(S, dtype=torch.float32, device="cuda")
    dh.set_option("attn_mask_force", 1)
    try:
        dh.attention_fwd_masked(qkv, o, lse, plan, B, H, S)
    finally:
        dh.set_option("attn_mask_force", 0)
    assert torch.equal(o[0].cpu(), qkv[0, 2 * HD:].cpu())


def test_deterministic_with_reserved_cus():
    m = pattern_mask("conv:3", 16, 256)
    outs = []
    for reserve in (0, 0, 16):
        dh.set_option("reserve_cus", reserve)
        try:
            _, _, _, o, lse, dqkv = _check(m, B=2, H=4, seed=8)
        finally:
            dh.set_option("reserve_cus", 0)
        outs.append((o, lse, dqkv))
    for o, lse, dqkv in outs[1:]:
        assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1]) and torch.equal(dqkv, outs[0][2])


@pytest.mark.parametrize("pattern", ["row", "column", "conv:3", "local:40"])
def test_decode_matches_forward_rows(pattern):
    """decode against the masked forward at every position: by value, from pos_dev, from a `fresh` staging row, and as one
    captured graph replayed across positions"""
    B, H, T, P = 2, 2, 16, 256
    S = T + P
    m = pattern_mask(pattern, T, P)
    plan = dh.AttnMaskPlan(m)
    qkv = _qkv(B, H, S, 9)
    o = torch.empty(B * S, H * HD, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B * H * S, dtype=torch.float32, device="cuda")
    dh.attention_fwd_masked(qkv, o, lse, plan, B, H, S)
    ref = o.view(B, S, -1)
    od = torch.empty(B, H * HD, dtype=torch.bfloat16, device="cuda")
    pos_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    for pos in range(S):
        dh.attention_decode_masked(qkv, od, plan, B, H, S, pos)
        close(od, ref[:, pos], 1.6e-2, 1.5e-2, f"decode at {pos}")
    # fresh + pos_dev, captured once and replayed for a run of positions: the cache rows come from the staging buffer
    cache = qkv.clone()
    q3 = qkv.view(B, S, -1)
    fresh = torch.empty(B, 3 * H * HD, dtype=torch.bfloat16, device="cuda")
    outs = torch.empty(S, B, H * HD, dtype=torch.bfloat16, device="cuda")
    stream = torch.cuda.Stream()
    fresh.copy_(q3[:, 0])                          # the warm-up launch rewrites cache row 0 with its own contents
    with torch.cuda.stream(stream):
        dh.attention_decode_masked(cache, od, plan, B, H, S, 0, fresh=fresh, pos_dev=pos_dev)   # warm-up
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            dh.attention_decode_masked(cache, od, plan, B, H, S, 0, fresh=fresh, pos_dev=pos_dev)
    torch.cuda.synchronize()
    cache.view(B, S, -1)[:, T:] = 0                 # image rows arrive only through `fresh`
    for pos in range(T, S):
        fresh.copy_(q3[:, pos])
        pos_dev.fill_(pos)
        graph.replay()
        outs[pos].copy_(od)
    torch.cuda.synchronize()
    for pos in range(T, S):
        close(outs[pos], ref[:, pos], 1.6e-2, 1.5e-2, f"graph decode at {pos}")
    assert torch.equal(cache, qkv)
