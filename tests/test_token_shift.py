"""Token shift on the CPU: the config key, the written-down source table against an explicit loop over the definition, the
float64 reference and its transpose against autograd, the shifted fp32 oracle's sanity (off = the plain oracle, causality), and the
ABI of the two entry points with their refusals."""
import ctypes

import numpy as np
import pytest
import torch

import dalle_hip as dh
import dalle_step_ref as sref
import token_shift_ref as tref
from src.dalle_mtf import token_shift as ts

X, Y, H = 0x10000, 0x20000, 0x30000       # fake device pointers: every refusal comes before a launch, none is dereferenced
INVALID = -1


# ------------------------------------------------------------------ config key
def test_resolve_off_and_on():
    assert ts.resolve_token_shift(None, 256, 256) is False
    assert ts.resolve_token_shift({}, 256, 256) is False
    assert ts.resolve_token_shift({"token_shift": None}, 256, 256) is False
    assert ts.resolve_token_shift({"token_shift": False}, 256, 256) is False
    assert ts.resolve_token_shift({"token_shift": True}, 256, 256) is True
    assert ts.resolve_token_shift({"token_shift": True}, 32, 1) is True
    # off asks nothing of the shape
    assert ts.resolve_token_shift({"token_shift": False}, 100, 250) is False


@pytest.mark.parametrize("bad", [1, "yes", 0.5, 0, "true", [True]])
def test_resolve_refuses_anything_but_a_bool(bad):
    with pytest.raises(ValueError, match="token_shift"):
        ts.resolve_token_shift({"token_shift": bad}, 256, 256)


def test_resolve_refuses_unfit_shapes():
    with pytest.raises(ValueError, match="token_shift.*perfect square"):
        ts.resolve_token_shift({"token_shift": True}, 256, 250)
    for d in (48, 100, 16, 0):
        with pytest.raises(ValueError, match="token_shift.*multiple of 32"):
            ts.resolve_token_shift({"token_shift": True}, d, 256)


def test_model_refuses_before_any_device_work():
    """DALLE raises on a machine without a GPU: the key is resolved before the engine is built"""
    from src.dalle_mtf.engine import DalleEngine
    from src.dalle_mtf.models import DALLE
    kw = dict(text_vocab_size=50, image_vocab_size=16, text_seq_len=8, n_layers=1, batch_size=1)
    for bad, n_embd, P in (("yes", 128, 16), (True, 128, 24), (True, 80, 16)):
        with pytest.raises(ValueError, match="token_shift"):
            DALLE(n_embd=n_embd, n_heads=2, image_seq_len=P, params={"token_shift": bad}, **kw)
        with pytest.raises(ValueError, match="token_shift"):
            DalleEngine(n_embd, 1, 2, 50, 16, 8, P, batch_size=1, hparams={"token_shift": bad})


# ------------------------------------------------------------------ the reference
def _loop(x, T, G):
    """the definition, position by position and channel by channel"""
    B, S, d = x.shape
    y = np.zeros_like(x)
    for b in range(B):
        for p in range(S):
            for ch in range(d):
                if ch >= d // 2:
                    y[b, p, ch] = x[b, p, ch]
                elif p < T:
                    y[b, p, ch] = x[b, p - 1, ch] if p >= 1 else 0.0
                else:
                    r, c = divmod(p - T, G)
                    if ch < d // 4:
                        y[b, p, ch] = x[b, p - G, ch] if r >= 1 else 0.0
                    else:
                        y[b, p, ch] = x[b, p - 1, ch] if c >= 1 else 0.0
    return y


@pytest.mark.parametrize("T,G", [(4, 6), (1, 6), (4, 1), (1, 1)])
def test_shift64_equals_the_definition(T, G):
    S, d, B = T + G * G, 32, 2
    x = np.random.default_rng(T * 10 + G).standard_normal((B, S, d))
    want = _loop(x, T, G)
    assert np.array_equal(tref.shift64(x.reshape(B * S, d), T, G).reshape(B, S, d), want)
    assert np.array_equal(tref.shift(torch.from_numpy(x), T, G).numpy(), want)
    src = ts.shift_sources(T, G, d)
    assert src.shape == (S, d) and src.dtype == np.int64
    pos = np.arange(S)[:, None]
    assert ((src < pos) | (src == pos)).all() and (src[:, d // 2:] == pos).all() and (src[:, :d // 2] < pos).all()   # causal
    assert (src[T:, :d // 2] < 0).sum() + (src[T:, :d // 2] >= T).sum() == src[T:, :d // 2].size        # image rows never read captions


@pytest.mark.parametrize("T,G", [(4, 6), (1, 6), (4, 1)])
def test_shift64_inverse_equals_the_autograd_transpose(T, G):
    S, d, B = T + G * G, 32, 2
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((B, S, d))).requires_grad_(True)
    dy = rng.standard_normal((B, S, d))
    tref.shift(x, T, G).backward(torch.from_numpy(dy))
    assert np.array_equal(tref.shift64(dy.reshape(B * S, d), T, G, inverse=True).reshape(B, S, d), x.grad.numpy())
    # and the adjoint identity, as sums of the same products
    xs = tref.shift64(x.detach().numpy().reshape(B * S, d), T, G)
    assert (xs * dy.reshape(B * S, d)).sum() == pytest.approx((x.detach().numpy() * x.grad.numpy()).sum(), rel=1e-12)


def _small():
    from oracle import dalle_oracle as do
    T, P, TV, IV = 8, 16, 50, 16
    cfg = do.DalleConfig(64, TV, IV, T, P, 2, 2)
    P0 = do.init_params(cfg, seed=5, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(2, T, TV, seed=1), do.synthetic_image_tokens(2, P, IV, seed=2), TV)
    return do, cfg, P0, tokens


def test_shift_off_reproduces_the_plain_oracle_exactly():
    do, cfg, P0, tokens = _small()
    loss_r, g_r = sref.loss_and_grads(P0, tokens, cfg, token_shift=False)
    loss_o, g_o = do.loss_and_grads(P0, tokens, cfg)
    assert loss_r == loss_o
    for k in g_o:
        assert np.array_equal(g_r[k], g_o[k]), k
    loss_x, g_x = sref.loss_and_grads(P0, tokens, cfg, token_shift=True)          # ... and the shift moves the loss and the gradients
    assert loss_x != loss_o and not np.array_equal(g_x["layer_0/attn/q"], g_o["layer_0/attn/q"])


def test_shifted_oracle_is_causal():
    """changing the token at position 100 leaves the logits before it bit-identical and changes those from it on"""
    from oracle import dalle_oracle as do
    T, P, TV, IV = 16, 256, 300, 64
    cfg = do.DalleConfig(128, TV, IV, T, P, 2, 2)
    P0 = {k: torch.tensor(v) for k, v in do.init_params(cfg, seed=1234, perturb=0.05).items()}
    tokens = do.assemble_tokens(do.synthetic_captions(1, T, TV, seed=1), do.synthetic_image_tokens(1, P, IV, seed=2), TV)
    other = tokens.copy()
    other[0, 100] = TV + (other[0, 100] - TV + 1) % IV
    with torch.no_grad():
        a = sref.forward_logits(P0, tokens, cfg, token_shift=True).numpy()
        b = sref.forward_logits(P0, other, cfg, token_shift=True).numpy()
    assert np.array_equal(a[:, :100], b[:, :100])
    after = np.abs(a[:, 100:] - b[:, 100:]).max(axis=-1)[0]
    assert after[0] > 0 and after[1] > 0 and after[16] > 0 and after.max() > 1e-3, after[:20]


# ------------------------------------------------------------------ ABI
def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_entry_points_are_declared_exported_and_bound():
    raw = ctypes.CDLL(dh.LIB_PATH)
    for name, nargs in (("dmi_token_shift", 10), ("dmi_token_shift_decode", 11)):
        assert name in dh.declared_symbols(), name
        assert hasattr(raw, name), name
        fn = getattr(dh.lib(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
        assert callable(getattr(dh, name[4:]))
    assert dh.lib().dmi_token_shift.argtypes[3] is ctypes.c_int64        # the row count travels whole


def test_refusals_come_before_any_launch():
    L = dh.lib()
    full = lambda x=X, y=Y, hist=None, rows=80, S=40, T=4, G=6, d=64, inverse=0: L.dmi_token_shift(x, y, hist, rows, S, T, G, d, inverse, None)   # noqa: E731
    dec = lambda x=X, hist=H, y=Y, B=2, S=40, T=4, G=6, d=64, pos=0, pos_dev=None: L.dmi_token_shift_decode(x, hist, y, B, S, T, G, d, pos, pos_dev, None)   # noqa: E731
    for call, prefix, ptrs, opt in ((full, "token_shift:", ("x", "y"), ("hist",)), (dec, "token_shift_decode:", ("x", "y", "hist"), ())):
        for p in ptrs:
            assert call(**{p: None}) == INVALID and _msg().startswith(prefix) and "null" in _msg(), (p, _msg())
        for p in ptrs + opt:
            assert call(**{p: 0x40000 + 8}) == INVALID and _msg().startswith(prefix) and "aligned" in _msg(), (p, _msg())
        assert call(S=0) == INVALID and _msg().startswith(prefix) and "empty" in _msg()
        assert call(d=0) == INVALID and _msg().startswith(prefix) and "empty" in _msg()
        for S in (39, 41, 36):
            assert call(S=S) == INVALID and _msg().startswith(prefix) and "T + G * G" in _msg(), (S, _msg())
        assert call(T=0, S=36) == INVALID and _msg().startswith(prefix) and "at least 1" in _msg()
        assert call(G=0, S=4) == INVALID and _msg().startswith(prefix) and "at least 1" in _msg()
        assert call(T=-32, G=6, S=4) == INVALID and _msg().startswith(prefix)
        for d in (16, 48, 72, 100):
            assert call(d=d) == INVALID and _msg().startswith(prefix) and "multiple of 32" in _msg(), (d, _msg())
        assert call(y=X) == INVALID and _msg().startswith(prefix) and "overlap" in _msg()
        assert call(y=X + 64) == INVALID and "overlap" in _msg()              # inside x's first row
    assert full(rows=0) == INVALID and "empty" in _msg()
    assert full(rows=-40) == INVALID
    for rows in (79, 41, 20):
        assert full(rows=rows) == INVALID and "multiple of S" in _msg(), (rows, _msg())
    assert full(y=X + 80 * 64 * 2 - 16) == INVALID and "overlap" in _msg()    # y starts in x's last row
    assert full(hist=H, inverse=1) == INVALID and "hist" in _msg()
    assert dec(B=0) == INVALID and "empty" in _msg()
    for pos in (-1, 40, 1 << 20):
        assert dec(pos=pos) == INVALID and "pos" in _msg(), (pos, _msg())
