"""QK normalisation on the CPU: the config key, the parameter layout with and without it, the ABI of the entry points and their
refusals, the float64 references against autograd, and the fp32 oracle's scale invariance and liveness."""
import ctypes

import numpy as np
import pytest
import torch

import dalle_hip as dh
import dalle_step_ref as sref
import qk_norm_ref as qref
from src.dalle_mtf import qk_norm as qn
from src.dalle_mtf.layout import ParamLayout, adafactor_table, reference_init

A, C, D = 0x10000, 0x20000, 0x30000       # fake device pointers: every refusal comes before a launch, none is dereferenced
INVALID, UNSUPPORTED = -1, -3


# ------------------------------------------------------------------ config key
def test_resolve_accepts_the_documented_values():
    assert qn.KEY == "qk_norm" and qn.EPS == 1e-6 == qref.EPS
    for off in (None, {}, {"qk_norm": None}, {"qk_norm": False}, {"rotary_emb": "1d"}):
        assert qn.resolve_qk_norm(off) is False
    assert qn.resolve_qk_norm({"qk_norm": True}) is True
    assert qn.q_scale(64) == 0.125 and qn.q_scale(128) == 128.0 ** -0.5


@pytest.mark.parametrize("bad", [1, 0, 1.0, "true", "rms", "", [True], {"eps": 1e-6}, np.bool_(True)])
def test_resolve_refuses_anything_but_a_bool(bad):
    with pytest.raises(ValueError, match="qk_norm"):
        qn.resolve_qk_norm({"qk_norm": bad})


def test_dalle_refuses_before_any_device_work():
    """a ValueError from DALLE.__init__, on a machine with or without a GPU: nothing was allocated or launched"""
    from src.dalle_mtf.engine import DalleEngine
    from src.dalle_mtf.models import DALLE
    kw = dict(n_embd=128, text_vocab_size=300, image_vocab_size=64, text_seq_len=16, image_seq_len=256, n_layers=1, n_heads=2, batch_size=1)
    for bad in (1, "on", 0.5):
        with pytest.raises(ValueError, match="qk_norm"):
            DALLE(params={"qk_norm": bad}, **kw)
        with pytest.raises(ValueError, match="qk_norm"):         # ... and from the engine itself, ahead of its device check
            DalleEngine(128, 1, 2, 300, 64, 16, 256, batch_size=1, hparams={"qk_norm": bad})


# ------------------------------------------------------------------ layout
@pytest.mark.parametrize("d,H", [(128, 2), (256, 2), (512, 4)])
def test_layout_off_is_todays(d, H):
    """the keyword absent and False: entries, offsets, total, transposed-copy table, bucket ends and ready points of the plain layout"""
    a, b = ParamLayout(d, 3, H, 365, 272), ParamLayout(d, 3, H, 365, 272, qk_norm=False)
    assert a.qk_norm is False and b.qk_norm is False
    assert a.entries == b.entries and a.offset == b.offset and a.total == b.total and a.t_offset == b.t_offset
    assert a.bucket_ends == b.bucket_ends and a.ready_points == b.ready_points
    assert not any("q_norm" in n or "k_norm" in n for n, _ in a.entries)
    assert len(a.entries) == 4 + 11 * 3 + 2
    on = ParamLayout(d, 3, H, 365, 272, qk_norm=True)
    plain = [(n, s) for n, s in on.entries if not n.endswith(qn.GAIN_NAMES)]
    assert plain == a.entries                           # on: the same entries in the same order, plus the gains


@pytest.mark.parametrize("d,H", [(128, 2), (256, 2)], ids=["hd64", "hd128"])
def test_layout_on_adds_two_gains_per_layer_between_qkv_and_norm_1(d, H):
    L, hd = 3, d // H
    off, on = ParamLayout(d, L, H, 365, 272), ParamLayout(d, L, H, 365, 272, qk_norm=True)
    names = [n for n, _ in on.entries]
    assert len(names) == len(off.entries) + 2 * L
    for i in range(L):
        at = names.index(f"layer_{i}/attn/qkv")
        assert names[at + 1:at + 4] == [f"layer_{i}/attn/q_norm/g", f"layer_{i}/attn/k_norm/g", f"layer_{i}/norm_1/g"]
        for g in qn.GAIN_NAMES:
            n = f"layer_{i}/{g}"
            assert on.shape[n] == (hd,) and on.offset[n] % 128 == 0          # 16-byte aligned in every flat buffer
            assert n not in on.t_offset
    assert on.total == off.total + 2 * L * 128                              # each [hd] gain takes one aligned slot
    # the cuts keep their meaning: a layer's bucket starts at its mlp_linear_2 kernel and holds its gains
    assert on.bucket_ends[0] == on.offset[f"layer_{L - 1}/mlp/mlp_linear_2/kernel"] and on.bucket_ends[-1] == on.total
    for bi, i in enumerate(reversed(range(L))):
        lo, hi = on.bucket_ends[bi], on.bucket_ends[bi + 1]
        assert all(lo <= on.offset[f"layer_{i}/{g}"] < hi for g in qn.GAIN_NAMES)
    assert on.ready_points == [on.offset["to_logits/layer_norm/g"]] + on.bucket_ends[1:]
    # the reference's variable table, Adafactor's and the initial values follow from the entries
    ref = {n: (s, o, ld) for n, s, o, ld in on.reference_variables()}
    table, recs, _ = adafactor_table(on)
    init = reference_init(on, H)
    for i in range(L):
        for g in qn.GAIN_NAMES:
            n = f"layer_{i}/{g}"
            assert ref[n] == ((hd,), on.offset[n], hd)
            rec = next(r for r in recs if r["name"] == n)
            assert rec["factored"] is False and rec["shape"] == (hd,)       # a 1-D variable: Adafactor keeps a dense v
            assert init[n].shape == (hd,) and init[n].dtype == np.float32 and np.array_equal(init[n], np.ones(hd, np.float32))
    assert set(reference_init(off, H)) == set(init) - {f"layer_{i}/{g}" for i in range(L) for g in qn.GAIN_NAMES}
    for n in reference_init(off, H):                                         # the draws of the other variables do not move
        assert np.array_equal(reference_init(off, H)[n], init[n]), n


def test_model_variables_list_the_gains():
    from src.dalle_mtf.models import DALLE
    m = DALLE.__new__(DALLE)
    from src.dalle_mtf.options import resolve_options
    m.n_embd, m.n_layers, m.n_heads, m.total_tokens, m.total_seq_dim = 128, 2, 2, 365, 272
    m.options = resolve_options({"ff_glu": False, "qk_norm": True}, 128, 16, 256)
    v = m.variables()
    assert v["layer_1/attn/q_norm/g"] == (64,) and v["layer_0/attn/k_norm/g"] == (64,)
    m.options = m.options._replace(qk_norm=False)
    assert "layer_1/attn/q_norm/g" not in m.variables()


# ------------------------------------------------------------------ ABI
def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_entry_points_are_declared_exported_and_bound():
    raw = ctypes.CDLL(dh.LIB_PATH)
    for name, nargs, res in (("dmi_qk_norm_fwd", 11, ctypes.c_int), ("dmi_qk_norm_bwd", 14, ctypes.c_int),
                             ("dmi_qk_norm_bwd_workspace_bytes", 2, ctypes.c_int64), ("dmi_qk_norm_decode", 11, ctypes.c_int)):
        assert name in dh.declared_symbols(), name
        assert hasattr(raw, name), name
        fn = getattr(dh.lib(), name)
        assert fn.restype is res and len(fn.argtypes) == nargs, name
        assert callable(getattr(dh, name[4:]))
    assert dh.lib().dmi_qk_norm_fwd.argtypes[6] is ctypes.c_int64 and dh.lib().dmi_qk_norm_bwd.argtypes[9] is ctypes.c_int64


def test_workspace_query_is_a_pure_host_function():
    """one partial row of 2 head_dim doubles per block of four rows, at most 2048 blocks; needs no device"""
    q = dh.qk_norm_bwd_workspace_bytes
    assert q(1, 64) == 2 * 64 * 8 and q(4, 128) == 2 * 128 * 8 and q(5, 128) == 2 * 2 * 128 * 8
    assert q(40960, 128) == 2048 * 2 * 128 * 8 == q(1 << 40, 128)
    assert q(0, 128) == 0


def test_refusals_come_before_any_launch():
    L = dh.lib()
    fwd = lambda qkv=A, ld=768, pre=None, gq=C, gk=D, cs=None, rows=8, S=4, H=2, hd=128: L.dmi_qk_norm_fwd(   # noqa: E731
        qkv, ld, pre, gq, gk, cs, rows, S, H, hd, None)
    bwd = lambda qkv=A, ld=768, pre=A + 0x4000, gq=C, gk=D, cs=None, dgq=C + 0x400, dgk=D + 0x400, ws=A + 0x8000, rows=8, S=4, H=2, hd=128: (   # noqa: E731
        L.dmi_qk_norm_bwd(qkv, ld, pre, gq, gk, cs, dgq, dgk, ws, rows, S, H, hd, None))
    dec = lambda qkv=A, gq=C, gk=D, cs=None, rows=2, S=4, H=2, hd=128, pos=0, pos_dev=None: L.dmi_qk_norm_decode(   # noqa: E731
        qkv, gq, gk, cs, rows, S, H, hd, pos, pos_dev, None)
    for call, prefix, required, nullable in ((fwd, "qk_norm_fwd:", ("qkv", "gq", "gk"), ("pre", "cs")),
                                             (bwd, "qk_norm_bwd:", ("qkv", "pre", "gq", "gk", "dgq", "dgk", "ws"), ("cs",)),
                                             (dec, "qk_norm_decode:", ("qkv", "gq", "gk"), ("cs",))):
        for p in required:
            assert call(**{p: None}) == INVALID and _msg().startswith(prefix) and "null" in _msg(), (p, _msg())
        for p in required + nullable:
            assert call(**{p: A + 8}) == INVALID and _msg().startswith(prefix) and "aligned" in _msg(), (p, _msg())
        for hd in (32, 96, 256, 0):
            assert call(hd=hd) == UNSUPPORTED and _msg().startswith(prefix) and "64 or 128" in _msg(), (hd, _msg())
        assert call(H=0) == INVALID and _msg().startswith(prefix)
        assert call(S=0) == INVALID and _msg().startswith(prefix) and "empty" in _msg()
        assert call(rows=0) == INVALID and call(rows=-4) == INVALID and "empty" in _msg()
    for call in (fwd, bwd):
        assert call(ld=504) == INVALID and "ld" in _msg()        # narrower than q | k
        assert call(ld=772) == INVALID and "ld" in _msg()        # rows would lose their 16-byte alignment
        assert call(hd=64, ld=248) == INVALID and "ld" in _msg()
    for pos in (-1, 4, 1 << 20):                                 # a by-value position matters with a table only
        assert dec(cs=A + 0x4000, pos=pos) == INVALID and "pos" in _msg(), (pos, _msg())


# ------------------------------------------------------------------ the float64 references
def _case(rng, rows, H, hd):
    x = rng.standard_normal((rows, 3 * H * hd))
    x[0, :hd] = 0.0                                              # an all-zero head
    x[1, 5] = 3.0e4
    gq, gk = rng.uniform(-2, 2, hd), rng.uniform(-2, 2, hd)
    gq[3] = 0.0
    return x, gq, gk


@pytest.mark.parametrize("rotary", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_float64_backward_equals_autograd_of_the_float64_forward(hd, rotary):
    """qk_norm_bwd64 against torch float64 autograd of the forward built from qk_norm_ref.normalise and rotary_ref.rotate (the
    functions the step oracle uses), which in turn equals qk_norm64: every tensor within 1e-12 relative (of its largest entry)"""
    from rotary_ref import rotate
    from src.dalle_mtf.rotary import rotary_table
    rng = np.random.default_rng(hd + rotary)
    B, S, H = 2, 40, 2
    rows, w = B * S, 2 * H * hd
    x, gq, gk = _case(rng, rows, H, hd)
    cs = rotary_table("axial", 4, 36, hd) if rotary else None
    dy = rng.standard_normal((rows, 3 * H * hd))
    xt = torch.tensor(x, requires_grad=True)
    gt = [torch.tensor(g, requires_grad=True) for g in (gq, gk)]
    halves = []
    for i, scale in enumerate((hd ** -0.5, 1.0)):
        t = xt[:, i * H * hd:(i + 1) * H * hd].reshape(B, S, H, hd).transpose(1, 2)
        t = qref.normalise(t, gt[i], scale)
        if rotary:
            t = rotate(t, torch.tensor(cs, dtype=torch.float64))
        halves.append(t.transpose(1, 2).reshape(rows, H * hd))
    y = torch.cat(halves, 1)
    y64 = qref.qk_norm64(x, gq, gk, H, hd, S, cs)
    assert np.array_equal(y64[:, w:], x[:, w:])
    assert np.abs(y.detach().numpy() - y64[:, :w]).max() <= 1e-12 * np.abs(y64[:, :w]).max()
    assert not np.isnan(y64).any() and np.array_equal(y64[0, :hd], np.zeros(hd))           # the all-zero head
    (y * torch.tensor(dy[:, :w])).sum().backward()
    dx, dgq, dgk, _, mag = qref.qk_norm_bwd64(dy, x, gq, gk, H, hd, S, cs)
    assert np.array_equal(dx[:, w:], dy[:, w:])
    for got, want in ((dx[:, :w], xt.grad.numpy()[:, :w]), (dgq, gt[0].grad.numpy()), (dgk, gt[1].grad.numpy())):
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), float(np.abs(got - want).max() / np.abs(want).max())
    assert (mag[0] >= np.abs(dgq)).all() and (mag[1] >= np.abs(dgk)).all()


# ------------------------------------------------------------------ the fp32 step oracle
def _small():
    from oracle import dalle_oracle as do
    T, P, TV, IV = 8, 16, 50, 16
    cfg = do.DalleConfig(128, TV, IV, T, P, 2, 2)
    P0 = do.init_params(cfg, seed=5, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(2, T, TV, seed=1), do.synthetic_image_tokens(2, P, IV, seed=2), TV)
    return cfg, P0, tokens


def test_scaling_wq_by_4_changes_the_logits_by_no_more_than_the_eps_term_allows():
    """With m = mean_j(q_j^2) of one head at one position, the normalised query of s q is s q / sqrt(s^2 m + eps) =
    [q / sqrt(m + eps)] sqrt((m + eps) / (m + eps / s^2)).  The last factor is sqrt(1 + t) with t = eps (1 - 1 / s^2) /
    (m + eps / s^2) < eps / m, and sqrt(1 + t) - 1 <= t / 2: every normalised query, and so every attention logit of its row,
    changes by less than eps / (2 m) relative.  In fp32 the two evaluations also round differently: s = 4 scales x . Wq and m
    exactly, but m + eps, the rsqrt, the two products and the sum over the head's k channels each add at most one rounding,
    (k + 8) 2^-24 of sum_j |q'_j k'_j| in all.  Bound per logit: (eps / (2 m_min) + (k + 8) 2^-24) sum_j |q'_j| |k'_j|, m_min the
    row's own m.  Without the key the same scaling multiplies every logit by 4."""
    cfg, P0, _ = _small()
    k = cfg.n_embd // cfg.n_heads
    rng = np.random.default_rng(0)
    x = torch.tensor(rng.standard_normal((2, 24, cfg.n_embd)), dtype=torch.float32)
    Pg = qref.with_gains(P0, cfg, seed=1)
    wq, wk, gq, gk = (torch.tensor(Pg["layer_0/" + n]) for n in ("attn/q", "attn/k") + qref.GAINS)
    base = qref.attn_logits(x, wq, wk, gq, gk, cfg.n_heads)
    four = qref.attn_logits(x, 4.0 * wq, wk, gq, gk, cfg.n_heads)
    q = (x @ wq).view(2, 24, cfg.n_heads, k).transpose(1, 2)
    kk = (x @ wk).view(2, 24, cfg.n_heads, k).transpose(1, 2)
    m = (q.double() ** 2).mean(-1, keepdim=True)                                  # [B, H, S, 1]: one per logit row
    mag = qref.normalise(q, gq, k ** -0.5).abs().double() @ qref.normalise(kk, gk, 1.0).abs().double().transpose(-1, -2)
    bound = (qref.EPS / (2.0 * m) + (k + 8) * 2.0 ** -24) * mag
    err = (four.double() - base.double()).abs()
    print(f"attention logits under 4 Wq: worst change / bound {float((err / bound).max()):.3f}, largest eps term {float((qref.EPS / (2 * m)).max()):.2e}")
    assert (err <= bound).all(), float((err / bound).max())
    assert float(base.abs().max()) > 1.0                                          # logits of real size, not a bound met by zeros
    plain, plain4 = qref.attn_logits(x, wq, wk, None, None, cfg.n_heads), qref.attn_logits(x, 4.0 * wq, wk, None, None, cfg.n_heads)
    assert torch.equal(plain4, 4.0 * plain)


def test_the_key_is_live_in_the_oracle_with_all_gains_1():
    cfg, P0, tokens = _small()
    ones = qref.with_gains(P0, cfg, seed=0, noise=0.0)
    assert all(np.array_equal(ones[f"layer_{i}/{g}"], np.ones(64, np.float32)) for i in range(2) for g in qref.GAINS)
    loss_on, g_on = qref.loss_and_grads(ones, tokens, cfg)
    loss_off, g_off = sref.loss_and_grads(P0, tokens, cfg)
    assert abs(loss_on - loss_off) > 1e-4 * abs(loss_off), (loss_on, loss_off)
    assert set(g_on) == set(g_off) | {f"layer_{i}/{g}" for i in range(2) for g in qref.GAINS}
    for i in range(2):
        for g in qref.GAINS:
            assert np.abs(g_on[f"layer_{i}/{g}"]).max() > 0                        # the gains receive gradient
    assert not np.allclose(g_on["layer_0/attn/q"], g_off["layer_0/attn/q"], rtol=1e-2, atol=0)


def test_tf_checkpoint_carries_the_two_new_names(tmp_path):
    """the TF-checkpoint writer and reader work by variable name: the gains travel under layer_i/attn/{q,k}_norm/g"""
    from src.data.tf_checkpoint import load_model_variables, save_checkpoint
    lay = ParamLayout(128, 2, 2, 365, 272, qk_norm=True)
    init = reference_init(lay, 2)
    init["layer_1/attn/k_norm/g"] = (init["layer_1/attn/k_norm/g"] * np.arange(64, dtype=np.float32)).astype(np.float32)
    prefix = str(tmp_path / "model.ckpt-3")
    save_checkpoint(prefix, dict(init))
    back = load_model_variables(prefix)
    assert set(back) == set(init)
    for i in range(2):
        for g in qn.GAIN_NAMES:
            assert np.array_equal(back[f"layer_{i}/{g}"], init[f"layer_{i}/{g}"])
