"""The attention-backward references of tests/attention_bwd_ref.py, checked on the CPU: spec64 against float64 autograd, the bf16
emulation's own error against fixed caps (the yardstick must not drift loose), and the teeth of within_budget -- three seeded
faults it must reject, one of which the older elementwise assertion (2 % of the tensor's largest gradient) lets through."""
import numpy as np
import pytest
import torch

import attention_bwd_ref as ab
from masked_attention_ref import additive

FAMILIES = [("flat", None), ("warm", None), ("peaked", None)] + [("spike", s) for s in ab.SPIKES_520]


def _block_mask(S, seed, tile=32):
    """random 32 x 32 blocks plus scattered single entries under the causal triangle, diagonal kept (every row attends to itself)"""
    rng = np.random.default_rng(seed)
    nb = (S + tile - 1) // tile
    m = np.kron(rng.random((nb, nb)) < 0.5, np.ones((tile, tile), dtype=bool))[:S, :S] | (rng.random((S, S)) < 0.1)
    m &= np.tril(np.ones((S, S), dtype=bool))
    m[np.arange(S), np.arange(S)] = True
    return m


def _autograd(qkv, d_o, B, H, S, hd, mask, dtype):
    """(dq, dk, dv) [B, H, S, hd] by torch autograd of softmax(Q K^T + additive mask) V"""
    q, k, v = (t.to(dtype).clone().requires_grad_(True) for t in ab.split_heads(qkv, B, H, S, hd))
    m = torch.tril(torch.ones(S, S, dtype=torch.bool)).numpy() if mask is None else mask
    o = torch.softmax(q @ k.transpose(-1, -2) + additive(m).to(dtype), -1) @ v
    o.backward(d_o.to(dtype).view(B, S, H, hd).permute(0, 2, 1, 3))
    return q.grad, k.grad, v.grad


@pytest.mark.parametrize("B,H,S,hd,masked", [(2, 1, 40, 128, False), (1, 2, 72, 64, False), (1, 2, 72, 128, True)])
def test_spec64_equals_float64_autograd(B, H, S, hd, masked):
    """with o and lse taken exactly (the float64 forward) the spec IS the derivative of masked softmax attention"""
    mask = _block_mask(S, 3) if masked else None
    qkv, d_o = ab.family_qkv_do("warm", B, H, S, hd, seed=S)
    o, lse = ab.forward64(qkv, B, H, S, hd, mask)
    spec = ab.spec64(ab.make_inputs(qkv, o, lse, d_o, B, H, S, hd, mask))
    ref = _autograd(qkv, d_o, B, H, S, hd, mask, torch.float64)
    for nm, got, want in zip(("dq", "dk", "dv"), spec, ref):
        rel = float((got - want).abs().max() / want.abs().max())
        assert rel <= 1e-10, (nm, rel)
    assert float((spec[3] - (d_o.double() * o).view(B, S, H, hd).sum(-1).permute(0, 2, 1)).abs().max()) == 0.0


def _family_inputs(family, spike, hd):
    """the GPU tests' families with a modelled saved forward: the float64 forward's o rounded to bf16, its lse to fp32"""
    B, H, S = (1, 1, 520) if spike is not None else (2, 2, 272)
    qkv, d_o = ab.family_qkv_do(family, B, H, S, hd, seed=S + hd, spike=spike)
    o, lse = ab.forward64(qkv, B, H, S, hd)
    return ab.make_inputs(qkv, o.to(torch.bfloat16), lse.float(), d_o, B, H, S, hd)


_CACHE = {}


def _cached(family, spike, hd):
    key = (family, spike, hd)
    if key not in _CACHE:
        _CACHE[key] = _family_inputs(family, spike, hd)
    return _CACHE[key]


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("family,spike", FAMILIES)
def test_emulation_stays_a_tight_yardstick(family, spike, hd):
    """the emulation's own dK / dV row error against the spec: at most 0.006, median at most 0.003, on every family (measured:
    0.0035 - 0.0044 and 0.0020 - 0.0023) -- every GPU bound is a multiple of these, so they must not drift loose"""
    _, _, err = ab.references(_cached(family, spike, hd))
    for nm in ("dk", "dv"):
        mx, med = float(err[nm].max()), float(err[nm].median())
        print(f"{family} {spike} hd {hd} {nm}: emulation row error max {mx:.4g} median {med:.4g}")
        assert mx <= 0.006 and med <= 0.003, (nm, mx, med)


def test_the_emulation_is_within_its_own_budget():
    inp = _cached("warm", None, 128)
    r = ab.within_budget(ab.emulated(inp), inp)
    assert all(v == (1.0, 1.0) for v in r.values()), r


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("fault", ab.FAULTS)
@pytest.mark.parametrize("family,spike", FAMILIES[:3] + FAMILIES[3:5])
def test_within_budget_rejects_seeded_faults(family, spike, fault, hd, capsys):
    """(a) the diagonal dS element of every 32nd query zeroed, (b) delta from the first half of the head dimension, doubled,
    (c) the last key of every 64-key chunk skipped in dV only: the function the GPU tests call refuses each, at their margins"""
    inp = _cached(family, spike, hd)
    with pytest.raises(AssertionError, match="over its error budget"):
        ab.within_budget(ab.emulated(inp, fault=fault), inp, 2.0, 1.5)
    assert "worst row (batch, head, position)" in capsys.readouterr().out


def test_diagonal_fault_rejected_on_todays_small_head_dim64_inputs():
    """head dim 64, S = 72, q * 0.12"""
    B, H, S, hd = 1, 1, 72, 64
    qkv, d_o = ab.family_qkv_do("flat", B, H, S, hd, seed=1)
    o, lse = ab.forward64(qkv, B, H, S, hd)
    inp = ab.make_inputs(qkv, o.to(torch.bfloat16), lse.float(), d_o, B, H, S, hd)
    with pytest.raises(AssertionError, match="dk"):
        ab.within_budget(ab.emulated(inp, fault="diag32"), inp, 2.0, 1.5)


def _old_assertion_passes(got, ref):
    """close(got, ref, 3e-2, 2e-2 * max|ref|) against fp32 autograd: every backward assertion the suite had"""
    err = (got.float() - ref).abs()
    return not bool((err > 2e-2 * float(ref.abs().max()) + 3e-2 * ref.abs()).any())


def test_the_old_assertion_passes_the_diagonal_fault_on_peaked_scores():
    """why the row metric exists: on the peaked family the fault of (a) leaves every element within 2 % of the largest gradient of
    its tensor, while a key row it hits (one whose diagonal P is not negligible) is ten times further off than any fault-free row
    (measured: 0.050 against 0.0046)"""
    inp = _cached("peaked", None, 128)
    B, H, S, hd = inp["B"], inp["H"], inp["S"], inp["hd"]
    ref = _autograd(inp["qkv"], inp["d_o"], B, H, S, hd, None, torch.float32)
    bad = ab.emulated(inp, fault="diag32")
    for nm, got, want in zip(("dq", "dk", "dv"), bad, ref):
        assert _old_assertion_passes(got, want), nm
    spec = ab.spec64(inp)
    hit = ab.row_error(bad[1], spec[1])[:, :, ::32]
    clean = ab.row_error(ab.emulated(inp)[1], spec[1])
    print(f"dk rows of the dropped diagonal: row error {float(hit.min()):.3g} .. {float(hit.max()):.3g}; fault-free max {float(clean.max()):.3g}")
    assert float(hit.max()) > 5 * float(clean.max()) and float(clean.max()) < 0.006
    with pytest.raises(AssertionError, match="over its error budget"):
        ab.within_budget(bad, inp, 2.0, 1.5)
