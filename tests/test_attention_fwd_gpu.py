"""Attention forward and decode kernels against their float64 specification under a per-row error budget
(tests/attention_fwd_ref.py), on flat, warm and peaked scores and with one spiked key.

Per case: every output starts as NaN; within_budget_fwd holds o (max / median row error against the float64 forward no more than
MARGIN_MAX / MARGIN_MED times the bf16 emulation's own) and lse (|lse - lse64| within the derived fp32 bound on every row).  Decode
is run at S = 1280, the smallest length at which one of the kernel's 16 waves takes a second 64-key chunk (the in-wave online-softmax
rescale with alpha != 1, and the masked instance's chunk skip in a second round), at chunk edges, the start of wave 0's and wave 1's
second chunk and the end; its rows are gathered over the positions and judged against float64 rows of the same bf16 cache, and the
`fresh` + `pos_dev` form must give the same bits and land the staging row in the cache.  Forward and decode with V scaled by 2^+-6
give 2^+-6 * o bit for bit and the same lse.

Head dim 64 takes the causal mask only: its masked case is the causal plan.

Measured on an MI355X: row error of the kernel's o over row error of the emulation, and over that of pure rounding bf16(o64), all
against the float64 forward (range over the group's cases; medians taken no smaller than 2^-10; every case prints its own RATIO
line: o/emulation max median | o/rounding max median | worst |lse - lse64| over its bound).

  group                                               cases   over the emulation               over pure rounding               lse /
                                                              max             median           max             median           bound
  attention_fwd hd 128, six shapes x three families,
      attn_fwd 1 (the software-pipelined kernel)         18   1.000 .. 1.466  1.000 .. 1.133   1.000 .. 1.826  1.000 .. 1.360   0.012
  the same, attn_fwd 0 (the program-order kernel)        18   0.946 .. 1.000  0.976 .. 1.000   1.000 .. 1.525  1.000 .. 1.236   0.011
  attention_fwd hd 64, six shapes x three families       18   0.887 .. 1.057  0.980 .. 1.000   1.000 .. 1.446  1.000 .. 1.325   0.029
  (4, 2, 272), attn_xcd 8 and 0, hd 128, three families   6   1.195 .. 1.370  1.012 .. 1.078   1.487 .. 1.732  1.036 .. 1.341   0.012
  the same, hd 64                                         6   0.874 .. 0.934  0.982 .. 0.990   1.176 .. 1.405  1.033 .. 1.296   0.022
  spiked key at S = 520, hd 128, attn_fwd 1               7   1.282 .. 1.326  1.009 .. 1.014   1.470 .. 1.523  1.029 .. 1.039   0.011
  the same, attn_fwd 0                                    7   0.972 .. 1.000  0.989 .. 0.993   1.108 .. 1.166  1.012 .. 1.016   0.011
  spiked key at S = 520, hd 64                            7   0.924 .. 1.000  0.985 .. 0.994   1.149 .. 1.253  1.015 .. 1.020   0.019
  attention_fwd_masked hd 128: local:40, row, conv:3,
      block, forced causal, three families each          15   0.920 .. 1.036  0.975 .. 0.999   1.103 .. 1.477  1.016 .. 1.229   0.012
  attention_fwd_masked hd 64, causal plan                 3   0.887 .. 1.000  0.986 .. 0.993   1.164 .. 1.382  1.025 .. 1.305   0.029
  decode (2, 2, 1280), hd 128 and 64, three families      6   0.888 .. 1.000  0.932 .. 0.995   1.109 .. 1.330  1.006 .. 1.269   -
  decode, three spiked keys, hd 128 and 64                6   0.890 .. 1.000  0.975 .. 1.000   1.020 .. 1.168  1.007 .. 1.049   -
  decode masked, row and conv:3, flat and peaked          4   0.947 .. 1.012  0.962 .. 1.000   1.051 .. 1.296  1.034 .. 1.178   -

Every group is inside the starting margins, 2.0 on the maximum and 1.5 on the median, so those are the margins in force;
tests/test_attention_fwd_ref.py proves that they reject a key dropped per 64-key chunk and a leaked key, and that the lse bound
rejects an lse taken from the bf16-rounded sum.  The program-order kernel, the head-dim-64 kernel, the masked kernel and decode
round the same fp32 values as the emulation (P = exp(s - rowmax) to bf16, normalised by the unrounded sum) and sit at 1.  The
software-pipelined kernel (attn_fwd 1) rounds P at the scale of an INTEGER base-2 maximum (P up to 2, not up to 1) and normalises by
the sum of the rounded P: its median stays at 1.01 .. 1.08 of the emulation's (1.13 at (1, 1, 8)), its worst row comes to 1.2 ..
1.47.  Against pure rounding its median on the peaked family is 1.00 .. 1.05 and the program-order kernel's 1.00 .. 1.04: the
1.05 and 1.02 of the kernel's header comment.  An experiment build of that kernel without the rounded sum (-DF2_LROUNDED=0) gave
1.22 .. 1.32 there (the header said 1.47 and now carries the measured figures) and FAILED this budget on the warm and peaked
families at (1, 1, 520), at 2.10 and 2.06 times the emulation's maximum: the design choice the header argues for is what keeps
the kernel inside the margin.  The worst lse of any kernel came to 0.029 of the derived bound (the fp32 emulation's own: 0.045),
and the power-of-two scaling of V is bit-exact on all seven paths.

The same budget is called on the o and lse of the older helpers (test_kernels_gpu.py::_attention_fwd_bwd, test_attn_mask_gpu.py::
_check, test_head_dim64_gpu.py::_vs_autograd), up to (8, 16, 1152): maximum 0.97 .. 1.32, 0.85 .. 1.00 and 0.93 .. 1.00 of the
emulation's, median 0.97 .. 1.08, lse at most 0.026 of its bound.
"""
import numpy as np
import pytest
import torch

import attention_fwd_ref as af
import dalle_hip as dh  # noqa: E402  (path set up by conftest)
from src.dalle_mtf.masks import pattern_mask

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN_MAX, MARGIN_MED = af.MARGIN_MAX, af.MARGIN_MED

SHAPES = [(1, 1, 8), (2, 1, 40), (1, 1, 72), (5, 2, 200), (2, 2, 272), (1, 1, 520)]
FAMILIES = ["flat", "warm", "peaked"]
# decode: chunk edges, the start of wave 0's second chunk (key 1024), of wave 1's (1088), and the end
DECODE_SHAPE = (2, 2, 1280)
DECODE_POSITIONS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 1087, 1088, 1279]
# (keyrow, qrow, mult): the maximum grows inside wave 0's second chunk; the maximum in the first round, the second negligible; the
# maximum in another wave (the cross-wave merge)
DECODE_SPIKES = [(1030, 1279, 3.0), (5, 1279, 3.0), (70, 1100, 2.0)]

_INPUTS = {}


def _block_mask(S, seed, tile=32):
    rng = np.random.default_rng(seed)
    nb = (S + tile - 1) // tile
    m = np.kron(rng.random((nb, nb)) < 0.5, np.ones((tile, tile), dtype=bool))[:S, :S] | (rng.random((S, S)) < 0.1)
    m &= np.tril(np.ones((S, S), dtype=bool))
    m[np.arange(S), np.arange(S)] = True
    return m


def _mask(name, S=272):
    if name is None:
        return None
    if name == "block":
        return _block_mask(S, 1)
    if name == "forced-causal":
        return np.tril(np.ones((S, S), dtype=bool))
    return pattern_mask(name, 16, 256) if S == 272 else pattern_mask(name, 256, 1024)


def _inputs(family, B, H, S, hd, spike=None, mask=None):
    """the inputs dict (bf16 qkv on the CPU, the mask, the cached references) of a (family, shape, mask name), drawn once and shared"""
    key = (family, B, H, S, hd, spike, mask)
    if key not in _INPUTS:
        qkv, _ = af.family_qkv_do(family, B, H, S, hd, seed=1000 * hd + S + B, spike=spike)
        _INPUTS[key] = af.make_inputs(qkv, B, H, S, hd, _mask(mask, S))
    return _INPUTS[key]


def _forward(qkv, B, H, S, hd, plan=None):
    """(o, lse); both start as NaN so that an element the kernel skips shows"""
    o = torch.full((B * S, H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    lse = torch.full((B, H, S), float("nan"), dtype=torch.float32, device=DEV)
    if plan is None:
        dh.attention_fwd(qkv, o, lse, B, H, S, head_dim=hd)
    else:
        dh.attention_fwd_masked(qkv, o, lse, plan, B, H, S, head_dim=hd)
    torch.cuda.synchronize()
    return o, lse


def _case(label, family, B, H, S, hd, spike=None, mask=None, force=False, arms=(None,), margins=(MARGIN_MAX, MARGIN_MED)):
    """forward (once per attn_fwd arm) and the verdicts; mask: a name of _mask, run through the masked entry point"""
    inp = _inputs(family, B, H, S, hd, spike, mask)
    qkv = inp["qkv"].to(DEV)
    plan = dh.AttnMaskPlan(inp["mask"].numpy()) if mask is not None else None
    dh.set_option("attn_mask_force", 1 if force else 0)
    try:
        for arm in arms:
            if arm is not None:
                dh.set_option("attn_fwd", arm)
            try:
                o, lse = _forward(qkv, B, H, S, hd, plan)
            finally:
                dh.set_option("attn_fwd", 1)
            af.within_budget_fwd(o, lse, inp, *margins, label=label + (f" attn_fwd={arm}" if arm is not None else ""))
    finally:
        dh.set_option("attn_mask_force", 0)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,H,S", SHAPES)
def test_fwd128_within_budget(B, H, S, family):
    """one partial tile; the sequence ending inside a tile with several (batch, head) items; one, a few and many key tiles -- on
    both attn_fwd arms, which round P at different scales and so need not agree bit for bit"""
    _case(f"hd128 {family} {(B, H, S)}", family, B, H, S, 128, arms=(1, 0))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("B,H,S", SHAPES)
def test_fwd64_within_budget(B, H, S, family):
    _case(f"hd64 {family} {(B, H, S)}", family, B, H, S, 64)


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("xcd", [8, 0])
@pytest.mark.parametrize("family", FAMILIES)
def test_fwd_both_item_schedules(family, xcd, hd):
    """(4, 2, 272): the (batch, head) count divides by 8 -- per-XCD item lists (attn_xcd 8) and one serpentine (0)"""
    dh.set_option("attn_xcd", xcd)
    try:
        _case(f"hd{hd} {family} (4, 2, 272) xcd={xcd}", family, 4, 2, 272, hd)
    finally:
        dh.set_option("attn_xcd", 8)


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("spike", af.SPIKES_520)
def test_fwd_spiked_key(spike, hd):
    """peaked scores plus one key far above everything its query saw before, in the first tile, in steady-state tiles and on the
    diagonal, in lower and upper half-row lanes: the deferred rescale after a maximum growth of more than 2^16 and a row maximum that
    must span both half rows"""
    _case(f"hd{hd} spike {spike}", "spike", 1, 1, 520, hd, spike=spike, arms=(1, 0) if hd == 128 else (None,))


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", ["local:40", "row", "conv:3", "block", "forced-causal"])
def test_fwd_masked_within_budget(name, family):
    _case(f"masked {name} {family}", family, 2, 2, 272, 128, mask=name, force=True)


@pytest.mark.parametrize("family", FAMILIES)
def test_fwd_masked_head_dim64_causal_plan(family):
    _case(f"masked hd64 causal plan {family}", family, 2, 2, 272, 64, mask="forced-causal")


# ------------------------------------------------------------------ decode

def _decode(qkv, B, H, S, hd, pos, plan=None, fresh=None, pos_dev=None):
    o = torch.full((B, H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
    if plan is None:
        dh.attention_decode(qkv, o, B, H, S, pos, fresh=fresh, pos_dev=pos_dev, head_dim=hd)
    else:
        dh.attention_decode_masked(qkv, o, plan, B, H, S, pos, fresh=fresh, pos_dev=pos_dev, head_dim=hd)
    return o


def _decode_case(label, family, hd, spike=None, mask=None):
    """every position of DECODE_POSITIONS by value and in the graph-replayable form, the rows gathered and judged together"""
    B, H, S = DECODE_SHAPE
    inp = _inputs(family, B, H, S, hd, spike, mask)
    qkv = inp["qkv"].to(DEV)
    plan = dh.AttnMaskPlan(inp["mask"].numpy()) if mask is not None else None
    assert plan is None or not plan.causal
    rows3 = qkv.view(B, S, 3 * H * hd)
    got = []
    for pos in DECODE_POSITIONS:
        o = _decode(qkv, B, H, S, hd, pos, plan)
        # position from device memory, q | k | v of the step handed over in a staging buffer: the same bits, and the staging row
        # lands in cache row pos
        cache = qkv.clone()
        cache.view(B, S, 3 * H * hd)[:, pos] = 0
        o2 = _decode(cache, B, H, S, hd, 0, plan, fresh=rows3[:, pos].contiguous(),
                     pos_dev=torch.tensor([pos], dtype=torch.int32, device=DEV))
        assert torch.equal(o2, o), f"{label}: fresh + pos_dev form differs at position {pos}"
        assert torch.equal(cache, qkv), f"{label}: staging row not in the cache at position {pos}"
        got.append(o)
    got = torch.stack(got, 1).reshape(B * len(DECODE_POSITIONS), H * hd)
    af.within_budget_fwd(got, None, inp, MARGIN_MAX, MARGIN_MED, rows=DECODE_POSITIONS, label=label)


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("family", FAMILIES)
def test_decode_within_budget(family, hd):
    _decode_case(f"decode hd{hd} {family}", family, hd)


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("spike", DECODE_SPIKES)
def test_decode_spiked_key(spike, hd):
    _decode_case(f"decode hd{hd} spike {spike}", "spike", hd, spike=spike)


@pytest.mark.parametrize("family", ["flat", "peaked"])
@pytest.mark.parametrize("name", ["row", "conv:3"])
def test_decode_masked_within_budget(name, family):
    """image positions attend to the 256 text keys and a few late image keys: whole chunks of a wave's first and second round are
    skipped"""
    _decode_case(f"decode masked {name} {family}", family, 128, mask=name)


# ------------------------------------------------------------------ exact scaling of V

@pytest.mark.parametrize("kind", ["fwd arm 1", "fwd arm 0", "fwd hd64", "fwd masked row", "decode hd128", "decode hd64", "decode masked row"])
def test_output_is_linear_in_v_bit_for_bit(kind):
    """o is linear in V, and every rounding on the way (P to bf16, fp32 accumulation of P V, the division by the sum, the bf16 store)
    commutes with an exact power-of-two scale while nothing leaves the normal range: forward(2^k V) is 2^k forward(V) bit for bit
    and lse does not move.  A difference means a term that does not carry V's scale."""
    decode = kind.startswith("decode")
    hd = 64 if "hd64" in kind else 128
    B, H, S = DECODE_SHAPE if decode else (2, 2, 272)
    mask = "row" if "masked" in kind else None
    inp = _inputs("warm", B, H, S, hd, None, mask)
    plan = dh.AttnMaskPlan(inp["mask"].numpy()) if mask is not None else None

    def run(qkv):
        if decode:
            return _decode(qkv, B, H, S, hd, S - 1, plan), None
        dh.set_option("attn_mask_force", 1 if mask is not None else 0)
        dh.set_option("attn_fwd", 0 if kind == "fwd arm 0" else 1)
        try:
            return _forward(qkv, B, H, S, hd, plan)
        finally:
            dh.set_option("attn_mask_force", 0)
            dh.set_option("attn_fwd", 1)

    base, lse0 = run(inp["qkv"].to(DEV))
    assert bool(torch.isfinite(base.float()).all())
    for k in (6, -6):
        f = 2.0 ** k
        t = inp["qkv"].clone().view(B * S, 3, H * hd)
        scaled = (t[:, 2].float() * f).to(torch.bfloat16)
        assert torch.equal(scaled.float(), t[:, 2].float() * f)
        t[:, 2] = scaled
        got, lse = run(t.view(B * S, 3 * H * hd).to(DEV))
        ne = got.float() != base.float() * f
        assert not bool(ne.any()), f"2^{k}: {int(ne.sum())}/{ne.numel()} elements differ, first at {ne.nonzero()[0].tolist()}"
        assert decode or torch.equal(lse, lse0), f"lse moves with V scaled by 2^{k}"
