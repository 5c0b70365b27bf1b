"""Gated feed-forward on the CPU (config key "ff_glu", DESIGN.md §4 "Gated feed-forward"): the float64 gate of tests/glu_ref.py against
torch autograd, the gated fp32 step oracle tied to the plain one, the config key, the parameter layout at the new width, and the
argument refusals of dmi_glu_fwd / dmi_glu_bwd."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dalle_hip as dh
import dalle_step_ref as sref
import glu_ref
from oracle import dalle_oracle as do
from src.dalle_mtf.ff_glu import ffn1_width, resolve_ff_glu
from src.dalle_mtf.layout import ParamLayout, adafactor_table, reference_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B_, C = 0x10000, 0x20000, 0x30000       # fake device pointers: every refusal comes before a launch, none is dereferenced
RELU, GELU = dh.GEMM_RELU, dh.GEMM_GELU


# ------------------------------------------------------------------ the float64 gate
@pytest.mark.parametrize("act", ["relu", "gelu"])
def test_glu_ref_matches_torch_autograd_in_float64(act):
    g = torch.Generator().manual_seed(5)
    gate = torch.cat([torch.linspace(-30, 30, 4001, dtype=torch.float64), torch.zeros(7, dtype=torch.float64),
                      torch.randn(1000, generator=g, dtype=torch.float64) * 3])
    assert (gate == 0).sum() >= 7
    n = gate.numel()
    val = torch.randn(n, generator=g, dtype=torch.float64) * 3
    dh_ = torch.randn(n, generator=g, dtype=torch.float64)
    pre = torch.cat([val, gate]).view(1, 2 * n)
    tf = (lambda x: torch.nn.functional.gelu(x, approximate="tanh")) if act == "gelu" else torch.relu
    leaf = pre.clone().requires_grad_(True)
    out = leaf[:, :n] * tf(leaf[:, n:])
    assert torch.allclose(glu_ref.glu(pre, act), out.detach(), rtol=1e-12, atol=1e-14)
    out.backward(dh_.view(1, n))
    got = glu_ref.glu_grad(dh_.view(1, n), pre, act)
    # (absolute term: far left 0.5 (1 + tanh u) cancels to a few float64 eps, 1.1e-16, where torch's form gives an exact 0; times
    # |dh * value| up to ~40 here)
    assert torch.allclose(got, leaf.grad, rtol=1e-12, atol=1e-13)
    if act == "relu":       # relu'(0) = 0, and the gate's gradient is an exact zero wherever the gate is not positive
        assert (got[0, n:][gate <= 0] == 0).all()
    # the numpy form computes the same
    assert np.allclose(glu_ref.glu(pre.numpy(), act), out.detach().numpy(), rtol=1e-12, atol=1e-14)
    assert np.allclose(glu_ref.glu_grad(dh_.view(1, n).numpy(), pre.numpy(), act), leaf.grad.numpy(), rtol=1e-12, atol=1e-13)


# ------------------------------------------------------------------ the gated step oracle, tied to the plain one
def _case():
    cfg = do.DalleConfig(128, 60, 16, 8, 16, 2, 1)
    P0 = do.init_params(cfg, seed=3, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(2, 8, 60, seed=1), do.synthetic_image_tokens(2, 16, 16, seed=2), 60)
    return cfg, P0, tokens


def test_reglu_with_an_open_gate_is_the_linear_mlp_and_ties_to_the_plain_oracle():
    """gate half of W1 zero, its bias 1: relu(gate) = 1 and h = value, a linear MLP.  (a) glu_ref's step equals the same step with a
    hand-written linear MLP -- (h W1v + b1v) W2 + b2 -- in loss and every gradient; (b) with the value bias at +8 every
    pre-activation is positive, so dalle_step_ref's ReLU MLP is that same linear map: the new oracle's loss and shared gradients
    equal the existing one's, which ties the composition around the MLP line to dalle_step_ref without editing it."""
    cfg, P0, tokens = _case()
    d = cfg.n_embd
    plain = {k: v.copy() for k, v in P0.items()}
    gated = {k: v.copy() for k, v in P0.items()}
    for i in range(cfg.n_layers):
        p = f"layer_{i}/mlp/mlp_linear_1/"
        plain[p + "bias"] = plain[p + "bias"] + np.float32(8.0)
        gated[p + "kernel"] = np.concatenate([plain[p + "kernel"], np.zeros((d, 4 * d), np.float32)], 1)
        gated[p + "bias"] = np.concatenate([plain[p + "bias"], np.ones(4 * d, np.float32)])
    loss_g, grads_g = glu_ref.loss_and_grads(gated, tokens, cfg, activation="relu")

    # (a) the hand-written linear MLP through the same composition
    P = sref.leaves(plain)
    tok = torch.as_tensor(tokens, dtype=torch.int64)
    x = P["embedding/wte"][tok] + P["positional_embedding/wpe"][:tok.shape[1]]
    for i in range(cfg.n_layers):
        p = f"layer_{i}/"
        h = do.layer_norm(x, P[p + "norm_1/g"], P[p + "norm_1/b"])
        x = x + sref.attention(h, P[p + "attn/q"], P[p + "attn/k"], P[p + "attn/v"], P[p + "attn/o"],
                               P[p + "attn/compute_output_bias/o_b"], cfg.n_heads, do.attn_mask(tok.shape[1]))
        h = do.layer_norm(x, P[p + "norm_2/g"], P[p + "norm_2/b"])
        a = h @ P[p + "mlp/mlp_linear_1/kernel"] + P[p + "mlp/mlp_linear_1/bias"]
        assert float(a.detach().min()) > 1.0                           # ... so the plain oracle's ReLU passes every element through
        x = x + a @ P[p + "mlp/mlp_linear_2/kernel"] + P[p + "mlp/mlp_linear_2/bias"]
    labels = torch.as_tensor(do.shift_labels(tokens, cfg.eos_token_id), dtype=torch.int64)
    loss_l = do.loss_fn(do.to_logits(P, x), labels)[0]
    grads_l = sref.gradients(loss_l, P)
    # (b) the existing oracle, whose ReLU never clips here
    loss_p, grads_p = sref.loss_and_grads(plain, tokens, cfg, activation="relu")
    for loss_o, grads_o in ((float(loss_l.detach()), grads_l), (loss_p, grads_p)):
        assert abs(loss_g - loss_o) <= 1e-6 * abs(loss_o), (loss_g, loss_o)
        for k, go in grads_o.items():
            gg = grads_g[k]
            if k.endswith("mlp_linear_1/kernel"):             # (the gate half has a gradient of its own, dh * value through relu'(1) = 1)
                assert np.abs(gg[:, 4 * d:]).max() > 0
                gg = gg[:, :4 * d]
            elif k.endswith("mlp_linear_1/bias"):
                gg = gg[:4 * d]
            err = np.linalg.norm(gg.astype(np.float64) - go) / (np.linalg.norm(go) + 1e-30)
            assert err <= 1e-4, (k, err)      # fp32 on both sides, other summation orders: the bound of the fp32 fixtures' comparisons


def test_widen_replaces_only_ffn1_and_the_gate_matters():
    cfg, P0, tokens = _case()
    P = glu_ref.widen(P0, cfg, seed=11)
    d = cfg.n_embd
    for k in P0:
        if "mlp_linear_1" in k:
            assert P[k].shape[-1] == 8 * d and P[k].dtype == np.float32 and np.abs(P[k]).max() > 0
        else:
            assert np.array_equal(P[k], P0[k])
    assert abs(float(P["layer_0/mlp/mlp_linear_1/kernel"].std()) - 0.02) < 1e-3
    assert np.array_equal(glu_ref.widen(P0, cfg, seed=11)["layer_1/mlp/mlp_linear_1/kernel"], P["layer_1/mlp/mlp_linear_1/kernel"])
    l_relu, g_relu = glu_ref.loss_and_grads(P, tokens, cfg, activation="relu")
    l_gelu, g_gelu = glu_ref.loss_and_grads(P, tokens, cfg, activation="gelu")
    assert l_relu != l_gelu
    for g in (g_relu, g_gelu):      # both halves of W1 and of b1 receive a gradient
        k, b = g["layer_0/mlp/mlp_linear_1/kernel"], g["layer_0/mlp/mlp_linear_1/bias"]
        assert np.abs(k[:, :4 * d]).max() > 0 and np.abs(k[:, 4 * d:]).max() > 0 and np.abs(b[:4 * d]).max() > 0 and np.abs(b[4 * d:]).max() > 0


# ------------------------------------------------------------------ the key
def test_resolve_off_and_on():
    assert resolve_ff_glu(None) is False and resolve_ff_glu({}) is False
    assert resolve_ff_glu({"ff_glu": None}) is False and resolve_ff_glu({"ff_glu": False}) is False
    assert resolve_ff_glu({"ff_glu": True}) is True
    assert ffn1_width(512, False) == 2048 and ffn1_width(512, True) == 4096


@pytest.mark.parametrize("bad", [1, "true", 0.5, 0, "yes", [True]])
def test_model_refuses_anything_but_a_bool_before_any_device_work(bad):
    """DALLE and DalleEngine raise on a machine without a GPU: the key is resolved before the engine touches a device"""
    from src.dalle_mtf.engine import DalleEngine
    from src.dalle_mtf.models import DALLE
    with pytest.raises(ValueError, match="ff_glu"):
        resolve_ff_glu({"ff_glu": bad})
    kw = dict(text_vocab_size=50, image_vocab_size=16, text_seq_len=8, image_seq_len=16, n_layers=1, batch_size=1)
    with pytest.raises(ValueError, match="ff_glu"):
        DALLE(n_embd=128, n_heads=2, params={"ff_glu": bad}, **kw)
    with pytest.raises(ValueError, match="ff_glu"):
        DalleEngine(128, 1, 2, 50, 16, 8, 16, batch_size=1, hparams={"ff_glu": bad})


@pytest.mark.parametrize("ok", [True, False, None, "absent"])
def test_model_accepts_the_bools_none_and_absent(ok):
    """a valid value passes the key's check: without a GPU the constructor then stops at the engine's device check, not at the key
    (with one, the GPU tests build such models)"""
    from src.dalle_mtf.models import DALLE
    params = {} if ok == "absent" else {"ff_glu": ok}
    assert resolve_ff_glu(params) is (ok is True)
    if not torch.cuda.is_available():
        with pytest.raises(dh.DalleHipError, match="HIP device"):
            DALLE(n_embd=128, n_heads=2, text_vocab_size=50, image_vocab_size=16, text_seq_len=8, image_seq_len=16, n_layers=1,
                  batch_size=1, params=params)


def test_shipped_configs_resolve_to_off():
    for name in os.listdir(os.path.join(ROOT, "configs")):
        cfg = json.load(open(os.path.join(ROOT, "configs", name)))
        assert resolve_ff_glu(cfg) is False, name


# ------------------------------------------------------------------ the layout
def test_layout_takes_the_ffn1_width_from_the_setting():
    d, L = 128, 2
    off, on = ParamLayout(d, L, 1, 77, 24), ParamLayout(d, L, 1, 77, 24, ff_glu=True)
    assert ParamLayout(d, L, 1, 77, 24, ff_glu=False).offset == off.offset and off.ffn1 == 4 * d and on.ffn1 == 8 * d
    assert on.total - off.total == L * (4 * d * d + 4 * d)         # 4 d^2 + 4 d more parameters per layer (both multiples of ALIGN)
    for i in range(L):
        k = f"layer_{i}/mlp/mlp_linear_1/"
        assert on.shape[k + "kernel"] == (d, 8 * d) and on.shape[k + "bias"] == (8 * d,)
        assert on.shape[f"layer_{i}/mlp/mlp_linear_2/kernel"] == (4 * d, d)
        assert on.t_offset[k + "kernel"] % 8 == 0 and (on.offset[k + "kernel"] * 2) % 16 == 0
    ref = {n: (s, ld) for n, s, _, ld in on.reference_variables()}
    assert ref["layer_1/mlp/mlp_linear_1/kernel"] == ((d, 8 * d), 8 * d) and ref["layer_1/mlp/mlp_linear_1/bias"] == ((8 * d,), 8 * d)
    # the transposed-copy table and Adafactor's follow the entries
    assert on.t_total - off.t_total == L * 4 * d * d
    rows = {r["name"]: r for r in adafactor_table(on)[1]}
    assert rows["layer_0/mlp/mlp_linear_1/kernel"]["shape"] == (d, 8 * d) and rows["layer_0/mlp/mlp_linear_1/kernel"]["factored"]
    # the reference's init at the new width: stddev 0.02, zero bias
    P = reference_init(on, 1, seed=7)
    w = P["layer_0/mlp/mlp_linear_1/kernel"]
    assert w.shape == (d, 8 * d) and abs(float(w.std()) - 0.02) < 5e-4 and not P["layer_0/mlp/mlp_linear_1/bias"].any()
    # off draws what it drew before the key existed
    assert np.array_equal(reference_init(off, 1, seed=7)["to_logits/linear_out/kernel"],
                          reference_init(ParamLayout(d, L, 1, 77, 24), 1, seed=7)["to_logits/linear_out/kernel"])


def test_dalle_variables_follow_the_key():
    from src.dalle_mtf.models import DALLE
    m = DALLE.__new__(DALLE)          # variables() reads the sizes alone: no engine, no device
    from src.dalle_mtf.options import resolve_options
    m.n_embd, m.n_layers, m.n_heads, m.total_tokens, m.total_seq_dim = 128, 1, 1, 77, 24
    m.options = resolve_options({}, 128, 8, 16)
    assert m.variables()["layer_0/mlp/mlp_linear_1/kernel"] == (128, 512)
    m.options = resolve_options({"ff_glu": True}, 128, 8, 16)
    assert m.variables()["layer_0/mlp/mlp_linear_1/kernel"] == (128, 1024) and m.variables()["layer_0/mlp/mlp_linear_1/bias"] == (1024,)


# ------------------------------------------------------------------ the C entry points
def _refused(rc, *words):
    msg = dh.lib().dmi_last_error_string().decode()
    assert rc == -1, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_glu_fwd_refuses_bad_arguments():
    f = dh.lib().dmi_glu_fwd
    M, Hh = 4, 64
    _refused(f(None, 128, B_, 64, M, Hh, RELU, None), "glu_fwd", "null pre")
    _refused(f(A, 128, None, 64, M, Hh, RELU, None), "glu_fwd", "null h")
    _refused(f(A, 128, B_, 64, M, 60, RELU, None), "glu_fwd", "Hh % 8")
    _refused(f(A, 128, B_, 64, M, 0, RELU, None), "glu_fwd", "Hh")
    _refused(f(A, 128, B_, 64, 0, Hh, RELU, None), "glu_fwd", "M > 0")
    _refused(f(A, 120, B_, 64, M, Hh, RELU, None), "glu_fwd", "ldpre")       # smaller than the row of 2 Hh
    _refused(f(A, 132, B_, 64, M, Hh, RELU, None), "glu_fwd", "ldpre")       # not a multiple of 8
    _refused(f(A, 128, B_, 56, M, Hh, RELU, None), "glu_fwd", "ldh")
    _refused(f(A, 128, B_, 68, M, Hh, RELU, None), "glu_fwd", "ldh")
    _refused(f(A + 8, 128, B_, 64, M, Hh, RELU, None), "glu_fwd", "pre must be 16-byte aligned")
    _refused(f(A, 128, B_ + 2, 64, M, Hh, RELU, None), "glu_fwd", "h must be 16-byte aligned")
    for act in (0, 1, dh.GEMM_RELU | dh.GEMM_GELU, dh.GEMM_RELU_MASK, -1):
        _refused(f(A, 128, B_, 64, M, Hh, act, None), "glu_fwd", "act")


def test_glu_bwd_refuses_bad_arguments():
    f = dh.lib().dmi_glu_bwd
    M, Hh = 4, 64
    _refused(f(None, 64, B_, 128, C, 128, M, Hh, GELU, None), "glu_bwd", "null dh")
    _refused(f(A, 64, None, 128, C, 128, M, Hh, GELU, None), "glu_bwd", "null pre")
    _refused(f(A, 64, B_, 128, None, 128, M, Hh, GELU, None), "glu_bwd", "null dpre")
    _refused(f(A, 64, B_, 128, C, 128, M, 12, GELU, None), "glu_bwd", "Hh % 8")
    _refused(f(A, 56, B_, 128, C, 128, M, Hh, GELU, None), "glu_bwd", "lddh")
    _refused(f(A, 68, B_, 128, C, 128, M, Hh, GELU, None), "glu_bwd", "lddh")
    _refused(f(A, 64, B_, 64, C, 128, M, Hh, GELU, None), "glu_bwd", "ldpre")
    _refused(f(A, 64, B_, 129, C, 128, M, Hh, GELU, None), "glu_bwd", "ldpre")
    _refused(f(A, 64, B_, 128, C, 127, M, Hh, GELU, None), "glu_bwd", "lddpre")
    _refused(f(A, 64, B_, 128, C, 132, M, Hh, GELU, None), "glu_bwd", "lddpre")
    _refused(f(A + 4, 64, B_, 128, C, 128, M, Hh, GELU, None), "glu_bwd", "dh must be 16-byte aligned")
    _refused(f(A, 64, B_ + 8, 128, C, 128, M, Hh, GELU, None), "glu_bwd", "pre must be 16-byte aligned")
    _refused(f(A, 64, B_, 128, C + 2, 128, M, Hh, GELU, None), "glu_bwd", "dpre must be 16-byte aligned")
    for act in (0, 3, dh.GEMM_BIAS, 1024):
        _refused(f(A, 64, B_, 128, C, 128, M, Hh, act, None), "glu_bwd", "act")


def test_python_wrappers_refuse_an_unknown_activation_before_the_library():
    with pytest.raises(dh.DalleHipError, match="'relu' or 'gelu'"):
        dh._glu_act("swish")
    assert dh._glu_act("relu") == dh.GEMM_RELU and dh._glu_act("gelu") == dh.GEMM_GELU
    assert {"dmi_glu_fwd", "dmi_glu_bwd"} <= set(dh.declared_symbols())
    assert isinstance(ctypes.c_void_p(A).value, int)
