"""GELU feed-forward on the CPU (DALLE activation_fn, DESIGN.md §4 "GELU"): the name resolution of DALLE(activation_fn=...) and the
config key, the float64 restatement tests/gelu_ref.py against torch, the reference's own DALLE with a GELU activation_fn
(tests/golden/ref_callsite_gelu.npz) against the fp32 step oracle with activation="gelu", and the argument checks of the two
new C entry points."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

import dalle_hip as dh

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
from gelu_ref import gelu, gelu_grad  # noqa: E402
from src.dalle_mtf.activations import ACTIVATIONS, check_activation, resolve_activation  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ref_callsite_gelu.npz")


# ------------------------------------------------------------------ names
def test_resolution_order_argument_then_config_key_then_relu():
    assert ACTIVATIONS == ("relu", "gelu")
    assert resolve_activation() == "relu"
    assert resolve_activation(None, {}) == "relu"
    assert resolve_activation(None, {"activation_fn": None}) == "relu"
    assert resolve_activation("gelu") == "gelu"
    assert resolve_activation("relu") == "relu"
    assert resolve_activation(None, {"activation_fn": "gelu"}) == "gelu"
    assert resolve_activation("relu", {"activation_fn": "gelu"}) == "relu"      # the argument wins
    assert resolve_activation("gelu", {"activation_fn": "relu"}) == "gelu"


@pytest.mark.parametrize("bad", ["swish", "GELU", "gelu_new", "", 3])
def test_unknown_names_are_refused_naming_the_supported_ones(bad):
    with pytest.raises(NotImplementedError, match="'relu' and 'gelu'"):
        resolve_activation(bad)
    with pytest.raises(NotImplementedError, match="'relu' and 'gelu'"):
        resolve_activation(None, {"activation_fn": bad})


def test_callables_are_refused():
    for fn in (torch.relu, lambda x: x, gelu):
        with pytest.raises(NotImplementedError, match="callable"):
            check_activation(fn)


def test_dalle_constructor_refuses_before_building_the_engine():
    """the checks run before any device work, so they hold on a machine without a GPU too"""
    from src.dalle_mtf.models import DALLE
    with pytest.raises(NotImplementedError, match="'relu' and 'gelu'"):
        DALLE(256, n_heads=2, activation_fn="swish")
    with pytest.raises(NotImplementedError, match="'relu' and 'gelu'"):
        DALLE(256, n_heads=2, params={"activation_fn": "tanh"})
    with pytest.raises(NotImplementedError, match="callable"):
        DALLE(256, n_heads=2, activation_fn=torch.relu)
    with pytest.raises(NotImplementedError, match="loss_fn"):
        DALLE(256, n_heads=2, activation_fn="gelu", loss_fn=lambda *a: 0)


def test_shipped_configs_keep_relu():
    for name in os.listdir(os.path.join(ROOT, "configs")):
        cfg = json.load(open(os.path.join(ROOT, "configs", name)))
        assert resolve_activation(None, cfg) == "relu", name


# ------------------------------------------------------------------ the float64 restatement
def test_gelu_ref_matches_torch_tanh_gelu_and_autograd():
    x = torch.cat([torch.linspace(-30, 30, 20001, dtype=torch.float64), torch.randn(5000, dtype=torch.float64) * 3])
    ref = torch.nn.functional.gelu(x, approximate="tanh")
    assert torch.allclose(gelu(x), ref, rtol=1e-13, atol=1e-15)
    xr = x.clone().requires_grad_(True)
    torch.nn.functional.gelu(xr, approximate="tanh").sum().backward()
    assert torch.allclose(gelu_grad(x), xr.grad, rtol=1e-12, atol=1e-14)
    # numpy form, and the identity gelu(x) = x * sigmoid(2u) the kernels evaluate
    xn = x.numpy()
    assert np.allclose(gelu(xn), ref.numpy(), rtol=1e-13, atol=1e-15)
    u = np.sqrt(2 / np.pi) * (xn + 0.044715 * xn ** 3)
    with np.errstate(over="ignore"):       # exp(-2u) = inf far left: x / inf = -0, the saturation the kernels rely on
        assert np.allclose(xn / (1 + np.exp(-2 * u)), ref.numpy(), rtol=1e-12, atol=1e-15)


def test_kernel_constants_match_the_formula():
    """the folded constants of gemm.hip's gelu_sig / gelu_grad_f"""
    src = open(os.path.join(ROOT, "dalle-mtf_amd", "csrc", "gemm.hip")).read()
    k0, log2e = np.sqrt(2 / np.pi), 1 / np.log(2)
    for name, val in (("C0", 2 * k0 * log2e), ("C1", 2 * k0 * 0.044715 * log2e), ("D0", 2 * k0), ("D1", 6 * k0 * 0.044715)):
        lit = src.split(f"constexpr float {name} = ")[1].split("f;")[0]
        assert abs(float(lit) - val) <= 1e-15 * val, (name, lit, val)


# ------------------------------------------------------------------ the reference's call site
def _fixture():
    blob = np.load(GOLDEN, allow_pickle=False)
    return blob, json.loads(str(blob["case"]))


def test_fixture_is_small():
    assert os.path.getsize(GOLDEN) < 400 * 1024


def test_reference_gelu_dalle_matches_the_gelu_oracle():
    """the reference's DALLE(activation_fn=<gelu>) over the shims, one step of a small model (tests/golden/make_gelu_golden.py),
    against the fp32 step oracle (tests/dalle_step_ref.py) with activation="gelu": loss and every gradient (float32 on both sides)"""
    import dalle_step_ref as sref
    from oracle import dalle_oracle as do
    blob, case = _fixture()
    cfg = do.DalleConfig(*[case[k] for k in ("n_embd", "text_vocab_size", "image_vocab_size", "text_seq_len", "image_seq_len",
                                               "n_layers", "n_heads")])
    P0 = do.init_params(cfg, seed=case["seed"], perturb=case["perturb"])
    tokens = blob["tokens"]
    _, grads_relu = do.loss_and_grads(P0, tokens, cfg)
    loss, grads = sref.loss_and_grads(P0, tokens, cfg, activation="gelu")
    ref_loss = float(blob["loss"])
    assert abs(loss - ref_loss) <= 2e-6 * abs(ref_loss), (loss, ref_loss)
    k1 = "layer_0/mlp/mlp_linear_1/kernel"      # the fixture tells GELU from ReLU
    r1 = blob["grad:" + k1].astype(np.float64)
    assert np.linalg.norm(grads_relu[k1] - r1) > 0.05 * np.linalg.norm(r1)
    names = [k[len("grad:"):] for k in blob.files if k.startswith("grad:")]
    assert set(names) == set(grads), sorted(set(names) ^ set(grads))
    for k in names:
        g, r = grads[k].astype(np.float64), blob["grad:" + k].astype(np.float64)
        rel = np.linalg.norm(g - r) / (np.linalg.norm(r) + 1e-30)
        assert rel <= 1e-4, (k, rel)


# ------------------------------------------------------------------ the C entry points
def test_gelu_entry_points_refuse_bad_arguments():
    L = dh.lib()
    buf = ctypes.c_void_p(0x10000)          # never dereferenced: every call below is refused before a launch
    rc = L.dmi_gemm_nt_gelu(buf, 128, buf, 128, buf, 256, 64, 256, 128, buf, None, 256, None)
    assert rc == -1 and "null pre" in L.dmi_last_error_string().decode()
    rc = L.dmi_gemm_nt_gelu(buf, 128, buf, 128, buf, 256, 64, 256, 128, None, buf, 256, None)
    assert rc == -1 and "null bias" in L.dmi_last_error_string().decode()
    rc = L.dmi_gemm_nt_gelu(buf, 128, buf, 128, buf, 256, 64, 256, 128, buf, ctypes.c_void_p(0x10008), 256, None)
    assert rc == -1 and "aligned" in L.dmi_last_error_string().decode()
    rc = L.dmi_gemm_nt_gelu(buf, 128, buf, 128, buf, 256, 64, 256, 128, buf, buf, 248, None)
    assert rc == -1 and "ldpre" in L.dmi_last_error_string().decode()
    rc = L.dmi_gemm_nt_gelu_grad(buf, 128, buf, 128, buf, 256, 64, 256, 128, buf, 260, None)
    assert rc == -1 and "ldpre" in L.dmi_last_error_string().decode()
    rc = L.dmi_gemm_nt_gelu_grad(buf, 128, buf, 128, buf, 256, 64, 256, 128, None, 256, None)
    assert rc == -1 and "null pre" in L.dmi_last_error_string().decode()
    rc = L.dmi_gemm_nt_gelu_grad(None, 128, buf, 128, buf, 256, 64, 256, 128, buf, 256, None)
    assert rc == -1 and "gemm_nt" in L.dmi_last_error_string().decode()
    # GELU without BIAS is not a supported flag set of dmi_gemm_nt, and the decode path's LN + dense refuses it the same way
    rc = L.dmi_gemm_nt(buf, 128, buf, 128, buf, 256, 64, 256, 128, dh.GEMM_GELU, None, None, None, None, None)
    assert rc != 0 and "flag" in L.dmi_last_error_string().decode()
    rc = L.dmi_ln_gemm_nt(buf, 128, buf, buf, 1e-5, buf, 128, buf, 256, 4, 256, 128, dh.GEMM_GELU, None, None)
    assert rc != 0 and "flag" in L.dmi_last_error_string().decode()
    assert dh.GEMM_GELU == 512 and not dh.GEMM_GELU & (dh.GEMM_BIAS | dh.GEMM_RELU | dh.GEMM_RESIDUAL | dh.GEMM_RELU_MASK |
                                                       dh.GEMM_OUT_F32 | dh.GEMM_ROWSCALE | 64 | 128 | 256)
