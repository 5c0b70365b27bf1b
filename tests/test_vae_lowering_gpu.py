"""Oracle parity of the convolution arms that no shipped configuration reaches (the layer tests of
tests/test_vae_coco_parity_gpu.py run where every layer gathers implicitly), through the product's own dispatch
(DiscreteVAE._conv_fwd / _wgrad / _dgrad3 / _dgrad_down / _up_backward), batch 2, train mode:

  * "unaligned"  num_tokens 64, 16x16 images, convblocks [[2,16],[2,64]]: 8- and 16-channel layers, so the column matrix is
    materialised in every product, the forward keeps it for the weight gradient, 9 * 16 = 144 rows pad to the pitch 192, and the
    1x1 head gathers one tap;
  * "nonpow2"    num_tokens 64, 24x24 images, convblocks [[2,64],[2,128]]: grids 24 -> 12 -> 6, 64-aligned channels: the input
    gradients gather implicitly, the forward products and the weight gradients (dmi_conv_wgrad_tn needs power-of-two output
    dims) go through the column matrix.

One layer of each kind per configuration, against the fp32 oracle's restatement of tf.layers.conv2d / conv2d_transpose
(oracle/vae_oracle.py) on the SAME bf16-rounded inputs and weights, with the bounds of tests/vae_conv_parity.py.  The weight
gradient runs twice: right after the forward (on the kept column) and after `_col_valid.clear()` (column gathered again); the two
results are bit-equal.  The last test pins the scratch sizes of tests/golden/vae_lowering.json that need the library's
workspace functions."""
import functools
import json
import os

import pytest
import torch

import dalle_hip as dh
from oracle import vae_oracle as vo
import vae_conv_parity as vcp

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = {}
_check_bf16, _check_f32 = functools.partial(vcp.check_bf16, REPORT), functools.partial(vcp.check_f32, REPORT)
B = 2
CONFIGS = {"unaligned": dict(num_tokens=64, dimensions=16, convblocks=[[2, 16], [2, 64]]),
           "nonpow2": dict(num_tokens=64, dimensions=24, convblocks=[[2, 64], [2, 128]])}
# (configuration, layer, products that gather implicitly): "f" forward, "w" weight gradient, "d" input gradient
DOWN = [("unaligned", "encoder/block_0/layer_0/conv_downsample", ""),       # 3(8) -> 16 channels: nothing implicit
        ("nonpow2", "encoder/block_1/layer_0/conv_downsample", "d")]        # 64 -> 128, 12x12 -> 6x6
RES = [("unaligned", "encoder/block_0/layer_1/conv_in", ""),                # 16 channels at 8x8: K = 144 on the pitch 192
       ("unaligned", "encoder/block_0/layer_1/conv_out", ""),
       ("nonpow2", "encoder/block_0/layer_1/conv_in", "d"),                 # 64 channels at 12x12
       ("nonpow2", "encoder/block_0/layer_1/conv_out", "d")]
UP = [("unaligned", "decoder/block_1/layer_0/conv_upsample", "f"),          # 64 -> 16, 8x8 -> 16x16: dz has 16 channels
      ("nonpow2", "decoder/block_1/layer_0/conv_upsample", "f")]            # 128 -> 64, 12x12 -> 24x24: 64-aligned dz, 12x12 grid
FINAL = [("unaligned", ""), ("nonpow2", "")]                                # 16 channels: one-tap im2col; 64: the plain product


@pytest.fixture(scope="module")
def models():
    from src.vae_tf import DiscreteVAE
    made = {}

    def get(which):
        if which not in made:
            c = CONFIGS[which]
            P = vo.init_params(vo.VaeConfig(**c), seed=11, bias_perturb=0.05)
            vae = DiscreteVAE(batch_size=B, use_bf16=True, mode="train", **c)
            vae.load_reference_params(P)
            made[which] = (vae, P)
        return made[which]
    yield get
    made.clear()
    torch.cuda.empty_cache()


def _conv(vae, name):
    (c,) = [c for c in vae.convs if c.name == name]
    return c


def _p2(v):
    return v > 0 and (v & (v - 1)) == 0


def _padded(x, C):
    """[B,H,W,c] with zero channels up to C, as the [B*H*W, C] device operand"""
    out = torch.zeros(*x.shape[:3], C, dtype=x.dtype)
    out[..., :x.shape[3]] = x
    return out.to(DEV).view(-1, C)


def _wgrad_twice(vae, c, tag, fwd, x_dev, dy_dev, k, b):
    """the weight gradient on the column the forward kept (when it keeps one), then with the column gathered again: both against
    the oracle, and bit-equal to each other"""
    got = []
    for kept in (True, False):
        fwd()
        if not kept:
            vae._col_valid.clear()
        assert (c.name in vae._col_valid) == (kept and c.kind != "final" and not vae._implicit_ok(c))
        vae.g.zero_()
        vae._wgrad(c, x_dev, dy_dev)
        got.append((vae.view(vae.g, c.name + "/kernel").clone(), vae.view(vae.g, c.name + "/bias").clone()))
    vae._col_valid.clear()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    dW, db = got[0]
    _check_f32(tag + ":dW", dW[:, :c.cin_ref, :c.cout_ref].cpu(), k.grad)
    _check_f32(tag + ":db", db[:c.cout_ref].cpu(), b.grad)


@pytest.mark.parametrize("which,layer,implicit", DOWN)
def test_downsample_conv_vs_oracle(models, which, layer, implicit):
    vae, P = models(which)
    c = _conv(vae, layer)
    assert c.kind == "down" and not vae._implicit_ok(c) and ("d" in implicit) == (c.cout % 64 == 0)
    tag = which + "/" + layer
    x = vcp.rnd(B, c.H, c.W, c.cin_ref, seed=1)
    k, b = vcp.weights(vae, P, c)
    x_dev = _padded(x, c.cin)
    out = torch.empty(B * c.Ho * c.Wo, c.cout, dtype=torch.bfloat16, device=DEV)
    fwd = lambda: vae._conv_fwd(c, x_dev, out)
    fwd()
    xr = x.float().requires_grad_(True)
    ref = vo.conv2d_same(xr, k, b, 2)
    _check_bf16(tag + ":fwd", out.cpu().float(), ref.detach())
    dy = vcp.rnd(B, c.Ho, c.Wo, c.cout, seed=2)
    ref.backward(dy.float())
    dy_dev = dy.to(DEV).view(-1, c.cout)
    _wgrad_twice(vae, c, tag, fwd, x_dev, dy_dev, k, b)
    dx = torch.empty(B * c.H * c.W, c.cin, dtype=torch.bfloat16, device=DEV)
    vae._dgrad_down(c, dy_dev, dx)
    dx = dx.cpu().float().view(B, c.H, c.W, c.cin)
    _check_bf16(tag + ":dx", dx[..., :c.cin_ref], xr.grad)
    assert float(dx[..., c.cin_ref:].abs().max() if c.cin > c.cin_ref else 0.0) == 0.0      # zero kernel rows: zero gradient


@pytest.mark.parametrize("which,layer,implicit", RES)
def test_residual_conv_vs_oracle(models, which, layer, implicit):
    vae, P = models(which)
    c = _conv(vae, layer)
    assert c.kind == "res" and not vae._implicit_ok(c) and ("d" in implicit) == (c.cout % 64 == 0)
    tag = which + "/" + layer
    x = vcp.rnd(B, c.H, c.W, c.cin, seed=3)
    k, b = vcp.weights(vae, P, c)
    relu = layer.endswith("conv_in")
    res = vcp.rnd(B, c.H, c.W, c.cout, seed=4) if not relu else None
    x_dev = x.to(DEV).view(-1, c.cin)
    out = torch.empty(B * c.H * c.W, c.cout, dtype=torch.bfloat16, device=DEV)
    if relu:      # conv_in: bias + ReLU epilogue; conv_out: bias + residual epilogue
        fwd = lambda: vae._conv_fwd(c, x_dev, out, flags=dh.GEMM_RELU)
    else:
        res_dev = res.to(DEV).view(-1, c.cout)
        fwd = lambda: vae._conv_fwd(c, x_dev, out, flags=dh.GEMM_RESIDUAL, residual=res_dev)
    fwd()
    xr = x.float().requires_grad_(True)
    pre = vo.conv2d_same(xr, k, b, 1)
    ref = torch.relu(pre) if relu else pre + res.float()
    _check_bf16(tag + ":fwd", out.cpu().float(), ref.detach())
    dy = vcp.rnd(B, c.H, c.W, c.cout, seed=5)
    pre.backward(dy.float())
    dy_dev = dy.to(DEV).view(-1, c.cout)
    _wgrad_twice(vae, c, tag, fwd, x_dev, dy_dev, k, b)
    dx = torch.empty(B * c.H * c.W, c.cin, dtype=torch.bfloat16, device=DEV)
    vae._dgrad3(c, dy_dev, dx)
    _check_bf16(tag + ":dx", dx.cpu().float().view(B, c.H, c.W, c.cin), xr.grad)


@pytest.mark.parametrize("which,layer,implicit", UP)
def test_transposed_conv_vs_oracle(models, which, layer, implicit):
    vae, P = models(which)
    c = _conv(vae, layer)
    assert c.kind == "up" and ("f" in implicit) == (c.cin % 64 == 0)
    assert not (c.cout % 64 == 0 and _p2(c.H) and _p2(c.W))                 # the backward goes through the column matrix
    tag = which + "/" + layer
    x = vcp.rnd(B, c.H, c.W, c.cin, seed=6)
    k, b = vcp.weights(vae, P, c)                      # TF layout [kh,kw,Cout,Cin]
    x_dev = x.to(DEV).view(-1, c.cin)
    out = torch.empty(B * c.Ho * c.Wo, c.cout, dtype=torch.bfloat16, device=DEV)
    vae._conv_fwd(c, x_dev, out)
    xr = x.float().requires_grad_(True)
    ref = vo.conv2d_transpose_same(xr, k, b)
    _check_bf16(tag + ":fwd", out.cpu().float().view(B, c.Ho, c.Wo, c.cout), ref.detach())
    dz = vcp.rnd(B, c.Ho, c.Wo, c.cout, seed=7)
    ref.backward(dz.float())
    vae.g.zero_()
    dx = torch.empty(B * c.H * c.W, c.cin, dtype=torch.bfloat16, device=DEV)
    vae._up_backward(c, x_dev, dz.to(DEV).view(-1, c.cout), dx)
    _check_f32(tag + ":dW", vae.view(vae.g, c.name + "/kernel").cpu(), k.grad)
    _check_f32(tag + ":db", vae.view(vae.g, c.name + "/bias").cpu(), b.grad)
    _check_bf16(tag + ":dx", dx.cpu().float().view(B, c.H, c.W, c.cin), xr.grad)


@pytest.mark.parametrize("which,implicit", FINAL)
def test_head_1x1_conv_vs_oracle(models, which, implicit):
    """the reconstruction head: forward (one-tap im2col at 16 channels, the plain product at 64) and weight gradient; its column is
    never kept.  The pad channels of the output stay exactly zero."""
    vae, P = models(which)
    c = _conv(vae, "decoder/conv2d")
    assert c.kind == "final" and c.cout_ref == 3
    tag = which + "/" + c.name
    x = vcp.rnd(B, c.H, c.W, c.cin, seed=8)
    k, b = vcp.weights(vae, P, c)
    x_dev = x.to(DEV).view(-1, c.cin)
    out = torch.empty(B * c.H * c.W, c.cout, dtype=torch.bfloat16, device=DEV)       # cout = 64 padded channels
    fwd = lambda: vae._conv_fwd(c, x_dev, out)
    fwd()
    ref = vo.conv2d_same(x.float(), k, b, 1)
    _check_bf16(tag + ":fwd", out.cpu().float()[:, :3].reshape(B, c.H, c.W, 3), ref.detach())
    assert float(out[:, 3:].float().abs().max()) == 0.0
    dy = torch.zeros(B, c.H, c.W, c.cout, dtype=torch.bfloat16)
    dy[..., :3] = vcp.rnd(B, c.H, c.W, 3, seed=9)
    ref.backward(dy[..., :3].float())
    _wgrad_twice(vae, c, tag, fwd, x_dev, dy.to(DEV).view(-1, c.cout), k, b)


def test_workspace_sizes_match_the_recorded_ones():
    """ws, ws_cs and a ws_pool slot (sized through dmi_gemm_tn_workspace_bytes / dmi_colsum_workspace_bytes / dmi_mse_workspace_bytes)
    and the column scratch, for the five configurations of tests/golden/vae_lowering.json"""
    from src.vae_tf import DiscreteVAE
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "vae_lowering.json")))
    for name, G in golden.items():
        vae = DiscreteVAE(**G["config"])
        got = dict(ws_bytes=vae.ws.numel(), ws_cs_bytes=vae.ws_cs.numel(), ws_pool_slot_bytes=vae.ws_pool[0].numel(),
                   ws_pool_slots=len(vae.ws_pool), col_numel=vae.col.numel())
        assert got == {k: G[k] for k in got}, (name, got)
        del vae
    torch.cuda.empty_cache()
