"""The FP8 key/value cache kernels on the GPU.

dmi_kv8_quantize against tests/kv8_ref.py bit for bit (data and scale), over row ranges of a (2, 72, 2) buffer whose outputs start
as a pattern -- rows outside the range must keep it -- on inputs with planted zero rows and a row near 2^-126, and on inputs near
2^127.  This is also the check of whether gfx950's packed conversion is the OCP E4M3FN encoding torch implements.

dmi_attention_decode_kv8 at test_attention_fwd_gpu.py's DECODE_SHAPE and DECODE_POSITIONS: the cache is the reference quantisation
of a family's k | v, the float64 specification (attention_fwd_ref) runs on q and the DEQUANTISED cache -- bf16, exact -- and the
kernel's rows are held to within_budget_fwd with the project's margins: no new tolerance.  The staging row handed over is the
unquantised bf16 row.  At every position: the output bits do not depend on whether cache row pos was zero or already held the
reference quantisation, nor on the position coming by value or from device memory; afterwards the row equals the reference
quantisation bit for bit and no other row moved.

Measured on an MI355X (row error of the kernel's o over that of the bf16 emulation, both against the float64 forward on the
dequantised cache; every case prints its RATIO line): the six family cases maximum 0.83 .. 1.00, median 0.92 .. 1.00; the six
spiked cases 0.91 .. 1.00 and 0.95 .. 1.00; the four masked cases 0.91 .. 0.96 and 0.93 .. 1.00 -- inside the margins 2.0 / 1.5.
The quantiser's bytes and scales equal the reference's in all twelve cases: gfx950's packed conversion is torch's E4M3FN."""
import pytest
import torch

import attention_fwd_ref as af
import dalle_hip as dh  # noqa: E402  (path set up by conftest)
import kv8_ref
from src.dalle_mtf.masks import pattern_mask
from test_attention_fwd_gpu import DECODE_POSITIONS, DECODE_SHAPE, DECODE_SPIKES, FAMILIES

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN_MAX, MARGIN_MED = af.MARGIN_MAX, af.MARGIN_MED

# ------------------------------------------------------------------ quantiser
QB, QS, QH = 2, 72, 2
_QIN = {}


def _quant_inputs(kind, hd):
    """(qkv bf16 [B*S, 3d] on the CPU, reference data, reference scale), drawn once per (kind, head dim)"""
    if (kind, hd) not in _QIN:
        g = torch.Generator().manual_seed(hd + (0 if kind == "planted" else 1))
        x = torch.randn(QB, QS, 3, QH, hd, generator=g)
        if kind == "planted":
            x = x * torch.exp2(torch.randint(-12, 12, (QB, QS, 3, QH, 1), generator=g).float())
            x[0, 0, 1, 0] = 0                       # zero rows: the first row, a row inside, a v row at the end of a range
            x[1, 5, 1, 1] = 0
            x[1, 71, 2, 0] = 0
            x[0, 5, 2, 1] *= 2.0 ** -126            # near 2^-126: the maximum a small normal, most of the row subnormal in bf16
            x[1, 63, 1, 0] *= 2.0 ** -128
            x[0, 70, 1, 1, 1:] = 0                  # one value alone, and one tiny value alone (the exponent's lower clamp)
            x[0, 71, 2, 1] = 0
            x[0, 71, 2, 1, 9] = -1.0e-38
        else:
            x = x * 2.0 ** 125                      # near 2^127: maxima up to 1.x * 2^127, the exponent's upper clamp
            x = x.clamp(-3.3e38, 3.3e38)
        qkv = x.to(torch.bfloat16).reshape(QB * QS, 3 * QH * hd)
        assert bool(torch.isfinite(qkv.float()).all())
        _QIN[(kind, hd)] = (qkv,) + kv8_ref.cache_of(qkv, QB, QS, QH, hd)
    return _QIN[(kind, hd)]


@pytest.mark.parametrize("s0,s1", [(0, 72), (5, 6), (63, 72)])
@pytest.mark.parametrize("kind", ["planted", "huge"])
@pytest.mark.parametrize("hd", [128, 64])
def test_quantiser_matches_the_reference_bit_for_bit(hd, kind, s0, s1):
    qkv, data_ref, scale_ref = _quant_inputs(kind, hd)
    data = torch.full((QB, QS, 2, QH, hd), 0xA5, dtype=torch.uint8, device=DEV)
    scale = torch.full((QB, QS, 2, QH), -7.0, dtype=torch.float32, device=DEV)
    dh.kv8_quantize(qkv.to(DEV), data, scale, QB, QS, QH, hd, s0, s1)
    torch.cuda.synchronize()
    data, scale = data.cpu(), scale.cpu()
    want_d, want_s = torch.full_like(data, 0xA5), torch.full_like(scale, -7.0)
    want_d[:, s0:s1], want_s[:, s0:s1] = data_ref[:, s0:s1], scale_ref[:, s0:s1]
    assert torch.equal(scale.view(torch.int32), want_s.view(torch.int32)), \
        f"scale differs at {(scale != want_s).nonzero()[:4].tolist()}"
    ne = data != want_d
    assert not bool(ne.any()), (f"{int(ne.sum())} bytes differ, first at {ne.nonzero()[0].tolist()}: "
                                f"got {int(data[ne][0]):#x}, reference {int(want_d[ne][0]):#x}")


# ------------------------------------------------------------------ decode
_INPUTS = {}


def _inputs(family, hd, spike=None, mask=None):
    """the family's bf16 qkv, its reference FP8 cache, and the inputs dict of the specification: q and the dequantised cache"""
    key = (family, hd, spike, mask)
    if key not in _INPUTS:
        B, H, S = DECODE_SHAPE
        qkv, _ = af.family_qkv_do(family, B, H, S, hd, seed=1000 * hd + S + B, spike=spike)
        data, scale = kv8_ref.cache_of(qkv, B, S, H, hd)
        deq = kv8_ref.dequantize(data, scale)
        assert torch.equal(deq.to(torch.bfloat16).float(), deq)
        spec = qkv.clone()
        spec.view(B, S, 3, H, hd)[:, :, 1:] = deq.to(torch.bfloat16)
        m = pattern_mask(mask, 256, 1024) if mask is not None else None
        _INPUTS[key] = dict(qkv=qkv, data=data, scale=scale, inp=af.make_inputs(spec, B, H, S, hd, m))
    return _INPUTS[key]


def _decode_case(label, family, hd, spike=None, mask=None):
    B, H, S = DECODE_SHAPE
    c = _inputs(family, hd, spike, mask)
    plan = dh.AttnMaskPlan(c["inp"]["mask"].numpy()) if mask is not None else None
    assert plan is None or not plan.causal
    rows3 = c["qkv"].view(B, S, 3 * H * hd).to(DEV)
    data_ref, scale_ref = c["data"].to(DEV), c["scale"].to(DEV)
    got = []
    for pos in DECODE_POSITIONS:
        fresh = rows3[:, pos].contiguous()
        outs = []
        for prefilled in (False, True):
            data, scale = data_ref.clone(), scale_ref.clone()
            if not prefilled:
                data[:, pos] = 0
                scale[:, pos] = 0
            o = torch.full((B, H * hd), float("nan"), dtype=torch.bfloat16, device=DEV)
            pos_dev = torch.tensor([pos], dtype=torch.int32, device=DEV) if prefilled else None     # by value, then from device memory
            dh.attention_decode_kv8(data, scale, fresh, o, B, H, S, 0 if prefilled else pos, pos_dev=pos_dev, head_dim=hd, plan=plan)
            assert torch.equal(data, data_ref), f"{label}: cache data differs from the reference quantisation after position {pos}"
            assert torch.equal(scale.view(torch.int32), scale_ref.view(torch.int32)), f"{label}: cache scale differs after position {pos}"
            outs.append(o)
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), \
            f"{label}: output depends on the old cache row / the form of the position at {pos}"
        got.append(outs[0])
    got = torch.stack(got, 1).reshape(B * len(DECODE_POSITIONS), H * hd)
    af.within_budget_fwd(got, None, c["inp"], MARGIN_MAX, MARGIN_MED, rows=DECODE_POSITIONS, label=label)


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("family", FAMILIES)
def test_decode_within_budget(family, hd):
    _decode_case(f"kv8 decode hd{hd} {family}", family, hd)


@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("spike", DECODE_SPIKES)
def test_decode_spiked_key(spike, hd):
    _decode_case(f"kv8 decode hd{hd} spike {spike}", "spike", hd, spike=spike)


@pytest.mark.parametrize("family", ["flat", "peaked"])
@pytest.mark.parametrize("name", ["row", "conv:3"])
def test_decode_masked_within_budget(name, family):
    _decode_case(f"kv8 decode masked {name} {family}", family, 128, mask=name)
