"""The attention-forward references of tests/attention_fwd_ref.py, checked on the CPU: the fp32 emulation stays inside the derived
lse bound on every family, shape and mask the GPU tests use (measured worst: 0.045 of it), the unfaulted emulation and the float64
output rounded to bf16 pass the budget, and within_budget_fwd has teeth -- it rejects three seeded faults where they apply."""
import math

import pytest
import torch

import attention_fwd_ref as af
from src.dalle_mtf.masks import pattern_mask

SHAPES = [(1, 1, 8), (2, 1, 40), (1, 1, 72), (5, 2, 200), (2, 2, 272), (1, 1, 520)]
DECODE_SPIKES = [(1030, 1279, 3.0), (5, 1279, 3.0), (70, 1100, 2.0)]

_CACHE = {}


def _inputs(family, B, H, S, hd, spike=None, mask=None):
    """inputs dict of a family, drawn once; mask = (name, text_len, image_len) of pattern_mask"""
    key = (family, B, H, S, hd, spike, mask)
    if key not in _CACHE:
        qkv, _ = af.family_qkv_do(family, B, H, S, hd, seed=1000 * hd + S + B, spike=spike)
        _CACHE[key] = af.make_inputs(qkv, B, H, S, hd, None if mask is None else pattern_mask(*mask))
    return _CACHE[key]


def _lse_over_bound(inp):
    _, lse64, _, el, bound, _ = af.references(inp)
    assert bool(torch.isfinite(el).all())
    return float(((el.double() - lse64).abs() / bound).max())


CASES = ([(f, B, H, S, hd, None, None) for f in ("flat", "warm", "peaked") for hd in (128, 64) for B, H, S in SHAPES]
         + [("spike", 1, 1, 520, hd, s, None) for hd in (128, 64) for s in af.SPIKES_520]
         + [(f, 2, 2, 272, 128, None, (name, 16, 256)) for f in ("flat", "warm", "peaked") for name in ("local:40", "row", "conv:3")]
         + [(f, 2, 2, 1280, hd, None, None) for f in ("flat", "warm", "peaked") for hd in (128, 64)]
         + [("spike", 2, 2, 1280, hd, s, None) for hd in (128, 64) for s in DECODE_SPIKES]
         + [(f, 2, 2, 1280, 128, None, (name, 256, 1024)) for f in ("flat", "peaked") for name in ("row", "conv:3")])


def test_emulation_stays_inside_the_lse_bound():
    """the bound is derived for ANY fp32 evaluation order, so torch's float32 forward must sit well inside it (measured: 0.045, on a
    spiked key at head dim 64)"""
    worst = (0.0, None)
    for case in CASES:
        r = _lse_over_bound(_inputs(*case))
        assert r <= 1.0, (case, r)
        worst = max(worst, (r, case), key=lambda t: t[0])
    print(f"emulation: worst |lse - lse64| / bound = {worst[0]:.3g} at {worst[1]} over {len(CASES)} cases")


@pytest.mark.parametrize("family", ["flat", "warm", "peaked"])
@pytest.mark.parametrize("B,H,S,hd", [(2, 2, 272, 128), (1, 1, 520, 64), (1, 1, 8, 128)])
def test_unfaulted_results_pass(B, H, S, hd, family):
    """the emulation against itself (ratios exactly 1) and the float64 result rounded once, with lse rounded to fp32"""
    inp = _inputs(family, B, H, S, hd)
    eo, el = af.emulated_forward(inp["qkv"], B, H, S, hd)
    r = af.within_budget_fwd(eo, el, inp, label=f"emulation {family} {(B, H, S, hd)}")
    assert r["emu"] == (1.0, 1.0) and r["lse"] <= 1.0
    o64, lse64 = af.references(inp)[:2]
    pure = o64.permute(0, 2, 1, 3).reshape(B * S, H * hd).to(torch.bfloat16)
    r = af.within_budget_fwd(pure, lse64.float(), inp, label=f"bf16(o64) {family} {(B, H, S, hd)}")
    assert r["rounding"][0] == 1.0 and r["emu"][0] <= 1.0 + 1e-9


def test_rows_select_positions():
    """decode's form: some positions only, no lse -- the same verdict as the full rows restricted to them"""
    B, H, S, hd = 2, 2, 272, 128
    inp = _inputs("warm", B, H, S, hd)
    eo, _ = af.emulated_forward(inp["qkv"], B, H, S, hd)
    rows = [0, 63, 64, 271]
    r = af.within_budget_fwd(eo.view(B, S, -1)[:, rows].reshape(B * len(rows), -1), None, inp, rows=rows)
    assert r["emu"] == (1.0, 1.0) and "lse" not in r
    bad, _ = af.emulated_forward(inp["qkv"], B, H, S, hd, fault="skip_key64")
    with pytest.raises(AssertionError, match=r"position\) = \(\d, \d, 271\)"):     # the only judged row past a chunk's last key
        af.within_budget_fwd(bad.view(B, S, -1)[:, rows].reshape(B * len(rows), -1), None, inp, rows=rows)


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("fault", ["skip_key64", "diag_leak"])
@pytest.mark.parametrize("B,H,S", [(2, 2, 272), (1, 1, 520)])
def test_o_maximum_rejects_chunk_and_mask_faults(B, H, S, fault, hd, capsys):
    """flat family (on peaked scores a leaked or dropped key often has negligible probability): rejected on the o MAXIMUM at the
    project's margins (measured: skip_key64 140 - 480 x the emulation's maximum, diag_leak 20 - 185 x)"""
    inp = _inputs("flat", B, H, S, hd)
    bad_o, bad_lse = af.emulated_forward(inp["qkv"], B, H, S, hd, fault=fault)
    r = af.within_budget_fwd(bad_o, None, inp, math.inf, math.inf)
    with capsys.disabled():
        print(f"\n{fault} flat {(B, H, S, hd)}: o max {r['emu'][0]:.1f} x the emulation's, median {r['emu'][1]:.2f} x")
    assert r["emu"][0] > af.MARGIN_MAX        # the maximum alone rejects it
    with pytest.raises(AssertionError, match="over its error budget"):
        af.within_budget_fwd(bad_o, bad_lse, inp, af.MARGIN_MAX, af.MARGIN_MED)
    assert "o: worst row (batch, head, position)" in capsys.readouterr().out


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("family", ["flat", "warm"])
@pytest.mark.parametrize("B,H,S", SHAPES)
def test_lse_bound_rejects_the_rounded_sum(B, H, S, family, hd, capsys):
    """lse from the sum of the bf16-rounded probabilities: o is untouched (ratios 1), the lse bound refuses it at every shape
    (measured: 1.8 - 64 x the bound)"""
    inp = _inputs(family, B, H, S, hd)
    o, lse = af.emulated_forward(inp["qkv"], B, H, S, hd, fault="lse_rounded_sum")
    with pytest.raises(AssertionError, match="lse: worst row"):
        af.within_budget_fwd(o, lse, inp, label=f"lse_rounded_sum {family} {(B, H, S, hd)}")
    out = capsys.readouterr().out
    assert "o/emulation 1.000 1.000" in out and "o: worst row" not in out
    with capsys.disabled():
        print("\n" + out.splitlines()[0])
