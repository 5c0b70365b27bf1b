"""Classifier-free guidance on the MI355X, the draw kernel alone: dmi_sample_tokens_guided against dmi_sample_tokens_p at scale 1,
against the numpy float32 restatement of g = zc + (scale - 1) (zc - zu) (tests/guidance_ref.py) for greedy draws, kept sets and
the drawn distribution, its logp against log_softmax of the conditional row, and the three ways of passing its settings."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guidance_ref import guided_keep, guided_logits, scaled  # noqa: E402

BC = 5
NVS = [64, 512, 2048, 8192]
_CACHE = {}


def _half(nv, seed, B=BC):
    """the row construction of test_generation_gpu._rows from a seed of its own (bias apart)"""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, nv + 8, generator=g) * 2).to(torch.bfloat16)
    z[1, 7] = z[1, 3] = z[1].float().max() + 1          # a tie of the maximum
    z[2, 20] = z[2, 10] = z[2].float().max() + 1
    z[3] = torch.round(z[3].float() / 2)                 # few distinct values: ties at tau
    return z, g


def _rows(nv):
    """z bf16 [2 Bc, nv + 8] (conditional rows first), bias bf16 [nv], zc / zu fp32 [Bc, nv] = z + bias.  Row 1 ties g exactly at
    its maximum for scale >= 1 (columns 3 and 7: equal and largest in zc, equal and smallest in zu), row 2 for scale <= 1
    (columns 10 and 20: equal and largest in both)."""
    if nv not in _CACHE:
        zc, g = _half(nv, nv + 1)
        bias = (torch.randn(nv, generator=g) * 0.5).to(torch.bfloat16)
        bias[7] = bias[3]
        bias[20] = bias[10]
        zu, _ = _half(nv, 7 * nv + 3)
        zu[1, 7] = zu[1, 3] = zu[1].float().min() - 2
        z = torch.cat([zc, zu])
        v = z[:, :nv].float() + bias.float()
        _CACHE[nv] = (z, bias, v[:BC].numpy().copy(), v[BC:].numpy().copy())
    return _CACHE[nv]


def _dev(nv):
    z, bias, zc, zu = _rows(nv)
    return z.cuda(), bias.cuda(), zc, zu


@pytest.mark.parametrize("nv", NVS)
def test_scale_one_is_the_nucleus_draw_on_the_conditional_rows(nv):
    import dalle_hip as dh
    zd, bd, _, _ = _dev(nv)
    o1 = torch.zeros(BC, 1, dtype=torch.int32, device="cuda")
    o2 = torch.zeros(BC, 1, dtype=torch.int32, device="cuda")
    nt = torch.full((2 * BC,), -1, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(nv)
    for it in range(60):
        T = [0.0, 0.5, 1.0, 1.7][it % 4]
        k = [0, 1, 6, nv // 3, nv][it % 5]
        p = [1.0, 0.9, 0.5][it % 3]
        seed, pos = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 20))
        dh.sample_tokens_p(zd, nv + 8, bd, BC, nv, temperature=T, top_k=k, seed=seed, top_p=p, pos=pos, out=o1, out_col0=pos)
        dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, temperature=T, top_k=k, seed=seed, top_p=p, scale=1.0, pos=pos,
                                token_offset=1000, next_tok=nt, out=o2, out_col0=pos)
        assert torch.equal(o1, o2), (T, k, p, seed, pos)
        assert torch.equal(nt[:BC], nt[BC:]) and torch.equal(nt[:BC], o2[:, 0] + 1000), (T, k, p, seed, pos)


@pytest.mark.parametrize("nv", NVS)
def test_greedy_is_the_first_maximum_of_the_restated_g(nv):
    import dalle_hip as dh
    zd, bd, zc, zu = _dev(nv)
    out = torch.zeros(BC, 1, dtype=torch.int32, device="cuda")
    nt = torch.zeros(2 * BC, dtype=torch.int32, device="cuda")
    for scale in (0.0, 0.5, 3.0, 7.5):
        g = guided_logits(zc, zu, scale)
        tied = [int((g[b] == g[b].max()).sum()) for b in range(BC)]
        assert max(tied) >= 2, (scale, tied)            # the construction: some row's maximum of g is an exact tie
        want = torch.from_numpy(np.argmax(g, -1).astype(np.int32))      # argmax returns the first maximum
        dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, temperature=0.0, top_k=3, top_p=0.2, scale=scale, pos=3, next_tok=nt,
                                out=out, out_col0=3)
        assert torch.equal(out[:, 0].cpu(), want), (scale, out[:, 0].cpu(), want)
        assert torch.equal(nt[:BC].cpu(), want) and torch.equal(nt[BC:].cpu(), want)


@pytest.mark.parametrize("nv", NVS)
def test_no_draw_outside_the_restated_kept_set(nv):
    import dalle_hip as dh
    zd, bd, zc, zu = _dev(nv)
    N = 1500
    for T, k, p, scale in ((1.0, 0, 0.9, 3.0), (0.7, 0, 0.5, 0.5), (1.3, 40, 0.8, 7.5), (1.0, 0, 1e-4, 0.0), (1.0, 7, 1.0, 2.0)):
        draws = torch.zeros(BC, N, dtype=torch.int32, device="cuda")
        for pos in range(N):
            dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, temperature=T, top_k=k, seed=11, top_p=p, scale=scale, pos=pos,
                                    out=draws, out_col0=0)
        draws = draws.cpu().numpy()
        for b in range(BC):
            keep = guided_keep(zc[b], zu[b], scale, T, k, p)
            assert keep[draws[b]].all(), (T, k, p, scale, b, int(keep.sum()))


@pytest.mark.parametrize("nv", NVS)
def test_draws_follow_the_renormalised_softmax_of_g_and_logp_scores_the_conditional_row(nv):
    import dalle_hip as dh
    zd, bd, zc, zu = _dev(nv)
    T, k, p, scale, N = 0.8, 0, 0.9, 3.0, 40000
    draws = torch.zeros(BC, N, dtype=torch.int32, device="cuda")
    for pos in range(N):
        dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, temperature=T, top_k=k, seed=9, top_p=p, scale=scale, pos=pos, out=draws,
                                out_col0=0)
    draws = draws.cpu().long()
    for b in range(BC):
        vb = torch.from_numpy(scaled(guided_logits(zc[b], zu[b], scale), T))
        keep = torch.from_numpy(guided_keep(zc[b], zu[b], scale, T, k, p))
        prob = torch.softmax(vb.double().masked_fill(~keep, float("-inf")), -1)
        freq = torch.bincount(draws[b], minlength=nv).double() / N
        assert bool((freq[~keep] == 0).all()), b
        sigma = torch.sqrt(prob * (1 - prob) / N)
        assert bool(((freq - prob).abs() <= 5 * sigma + 1e-4).all()), (b, float((freq - prob).abs().max()))
    # logp: log_softmax of the CONDITIONAL row (z + bias, fp32) at the drawn index, accumulated over calls
    lsm = torch.log_softmax(torch.from_numpy(zc), -1)
    o1 = torch.zeros(BC, 1, dtype=torch.int32, device="cuda")
    for T, k, p, scale in ((1.0, 0, 1.0, 3.0), (0.6, 5, 0.8, 7.5), (0.0, 0, 1.0, 0.5), (1.0, 0, 0.9, 0.0)):
        lp = torch.zeros(BC, dtype=torch.float32, device="cuda")
        want = torch.zeros(BC, dtype=torch.float64)
        for pos in range(3):
            dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, temperature=T, top_k=k, seed=5, top_p=p, scale=scale, pos=pos, out=o1,
                                    out_col0=pos, logp=lp)
            want += lsm[torch.arange(BC), o1[:, 0].cpu().long()].double()
        got = lp.cpu().double()
        assert bool(((got - want).abs() <= 2e-5 * (1 + want.abs())).all()), (T, k, p, scale, got, want)


@pytest.mark.parametrize("nv", NVS)
def test_by_value_params_dev_and_advance_give_the_same_draws(nv):
    import dalle_hip as dh
    zd, bd, _, _ = _dev(nv)
    T, k, p, scale, n = 0.8, 6, 0.7, 3.0, 6
    seed = (123 << 32) | 77
    ref = torch.zeros(BC, n, dtype=torch.int32, device="cuda")
    for pos in range(n):
        dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, temperature=T, top_k=k, seed=seed, top_p=p, scale=scale, pos=pos, out=ref,
                                out_col0=0)
    assert dh.sample_params(T, k, seed, top_p=p).tolist()[5] == 0            # the unguided block keeps its zero word
    prm = dh.sample_params(T, k, seed, top_p=p, guidance_scale=scale).cuda()
    assert prm.shape == (6,) and prm.cpu().numpy().view(np.uint32)[5] == np.array([scale], np.float32).view(np.uint32)[0]
    got = torch.zeros(BC, n, dtype=torch.int32, device="cuda")
    for pos in range(n):
        dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, params_dev=prm, pos_dev=torch.tensor([pos], dtype=torch.int32, device="cuda"),
                                out=got, out_col0=0)
    assert torch.equal(got, ref)
    pd = torch.tensor([0, 0], dtype=torch.int32, device="cuda")
    seq = torch.zeros(BC, n, dtype=torch.int32, device="cuda")
    nt = torch.zeros(2 * BC, dtype=torch.int32, device="cuda")
    for _ in range(n):
        dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, params_dev=prm, pos_dev=pd, advance=True, token_offset=7, next_tok=nt,
                                out=seq, out_col0=0)
    assert pd.cpu().tolist() == [n, 0] and torch.equal(seq, ref)
    assert torch.equal(nt[:BC], ref[:, n - 1] + 7) and torch.equal(nt[BC:], nt[:BC])
    # a different scale in the device block changes the draws somewhere (word 5 is read)
    prm2 = dh.sample_params(T, k, seed, top_p=p, guidance_scale=0.0).cuda()
    other = torch.zeros(BC, n, dtype=torch.int32, device="cuda")
    for pos in range(n):
        dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, params_dev=prm2, pos=pos, out=other, out_col0=0)
    byval = torch.zeros(BC, n, dtype=torch.int32, device="cuda")
    for pos in range(n):
        dh.sample_tokens_guided(zd, nv + 8, bd, BC, nv, temperature=T, top_k=k, seed=seed, top_p=p, scale=0.0, pos=pos, out=byval,
                                out_col0=0)
    assert torch.equal(other, byval) and not torch.equal(other, ref)
