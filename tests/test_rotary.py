"""Rotary position embeddings on the CPU: the config keys, the (cos, sin) table, its bands and position triples, the
relative-position property in float64, the ABI of the two entry points and their refusals, and the rotated fp32 oracle's sanity."""
import ctypes

import numpy as np
import pytest

import dalle_hip as dh
import dalle_step_ref as sref
import rotary_ref as rref
from src.dalle_mtf import rotary as ro

A, C = 0x10000, 0x20000       # fake device pointers: every refusal comes before a launch, none is dereferenced
INVALID, UNSUPPORTED = -1, -3


# ------------------------------------------------------------------ config keys
def test_resolve_accepts_the_documented_values():
    assert ro.resolve_rotary(None) == (None, 10000.0)
    assert ro.resolve_rotary({}) == (None, 10000.0)
    assert ro.resolve_rotary({"rotary_emb": None}) == (None, 10000.0)
    assert ro.resolve_rotary({"rotary_emb": False}) == (None, 10000.0)
    assert ro.resolve_rotary({"rotary_emb": "1d"}) == ("1d", 10000.0)
    assert ro.resolve_rotary({"rotary_emb": "axial", "rotary_base": 500}, 1024) == ("axial", 500.0)
    assert ro.resolve_rotary({"rotary_emb": "1d", "rotary_base": np.float32(1.5)}, 1000) == ("1d", 1.5)
    assert ro.resolve_rotary({"rotary_emb": "axial", "rotary_base": None}, 256) == ("axial", 10000.0)


@pytest.mark.parametrize("bad", [True, "2d", "AXIAL", "", 1, 0, 1.0, ["axial"], {"scheme": "1d"}])
def test_resolve_refuses_a_malformed_scheme(bad):
    with pytest.raises(ValueError, match="rotary_emb"):
        ro.resolve_rotary({"rotary_emb": bad}, 256)


@pytest.mark.parametrize("bad", [1, 1.0, 0.5, 0, -10000, float("inf"), float("nan"), "10000", True, [10000]])
def test_resolve_refuses_a_malformed_base(bad):
    with pytest.raises(ValueError, match="rotary_base"):
        ro.resolve_rotary({"rotary_emb": "1d", "rotary_base": bad}, 256)
    with pytest.raises(ValueError, match="rotary_base"):        # checked with the scheme off too
        ro.resolve_rotary({"rotary_base": bad}, 256)


def test_axial_needs_a_square_image_grid():
    for P in (255, 257, 1000, 2):
        with pytest.raises(ValueError, match="rotary_emb.*perfect square"):
            ro.resolve_rotary({"rotary_emb": "axial"}, P)
        ro.resolve_rotary({"rotary_emb": "1d"}, P)                # the flat scheme takes any length
        with pytest.raises(ValueError, match="perfect square"):
            ro.rotary_table("axial", 16, P, 64)


def test_dalle_refuses_before_any_device_work():
    """every refusal is a ValueError from DALLE.__init__, on a machine with or without a GPU: nothing was allocated or launched"""
    from src.dalle_mtf.models import DALLE
    kw = dict(n_embd=128, text_vocab_size=300, image_vocab_size=64, text_seq_len=16, n_layers=1, n_heads=2, batch_size=1)
    for params, P, match in (({"rotary_emb": "2d"}, 256, "rotary_emb"), ({"rotary_emb": True}, 256, "rotary_emb"),
                             ({"rotary_emb": "1d", "rotary_base": 1}, 256, "rotary_base"), ({"rotary_base": "x"}, 256, "rotary_base"),
                             ({"rotary_emb": "axial"}, 240, "perfect square")):
        with pytest.raises(ValueError, match=match):
            DALLE(image_seq_len=P, params=params, **kw)


# ------------------------------------------------------------------ table
def test_band_sizes():
    assert ro.band_sizes(128) == (22, 21, 21)
    assert ro.band_sizes(64) == (12, 10, 10)
    for hd in (64, 128):
        assert sum(ro.band_sizes(hd)) == hd // 2


@pytest.mark.parametrize("scheme", ro.SCHEMES)
@pytest.mark.parametrize("hd", [64, 128])
def test_table_shape_dtype_and_unit_norm(scheme, hd):
    T, P = 16, 256
    t = ro.rotary_table(scheme, T, P, hd)
    assert t.shape == (T + P, hd // 2, 2) and t.dtype == np.float32
    assert np.abs(t[..., 0].astype(np.float64) ** 2 + t[..., 1].astype(np.float64) ** 2 - 1.0).max() <= 1e-6
    a = ro.rotary_angles(scheme, T, P, hd)
    assert a.dtype == np.float64
    assert np.array_equal(t, np.stack([np.cos(a), np.sin(a)], -1).astype(np.float32))


def test_position_triples():
    T, P, G = 16, 256, 16
    pos = ro.position_triples(T, P)
    S = T + P
    want = {0: (0, 0, 0), T - 1: (T - 1, 0, 0), T: (T, 1, 1), T + G - 1: (T, 1, G), T + G: (T, 2, 1), S - 1: (T, G, G)}
    for s, w in want.items():
        assert tuple(pos[s]) == w, (s, tuple(pos[s]), w)


@pytest.mark.parametrize("hd", [64, 128])
def test_angles_are_band_component_times_frequency(hd):
    T, P, base = 16, 256, 10000.0
    n = hd // 2
    a1 = ro.rotary_angles("1d", T, P, hd, base)
    for s in (0, 1, T, T + P - 1):
        for c in (0, 1, n - 1):
            assert a1[s, c] == pytest.approx(s * base ** (-c / n), rel=1e-14, abs=0)
    ax = ro.rotary_angles("axial", T, P, hd, base)
    pos = ro.position_triples(T, P)
    nt, nr, nc = ro.band_sizes(hd)
    for s in (0, T - 1, T, T + 15, T + 16, T + P - 1):
        for band, (c0, m) in enumerate(((0, nt), (nt, nr), (nt + nr, nc))):
            for k in (0, 1, m - 1):
                assert ax[s, c0 + k] == pytest.approx(pos[s, band] * base ** (-k / m), rel=1e-14, abs=0)
    # the first pair of every band turns by the full component (frequency 1)
    assert np.array_equal(ax[:, 0], pos[:, 0]) and np.array_equal(ax[:, nt], pos[:, 1]) and np.array_equal(ax[:, nt + nr], pos[:, 2])
    # another base moves every pair but the first of a band
    assert not np.allclose(ro.rotary_angles("1d", T, P, hd, 100.0)[1, 1:], a1[1, 1:])


# ------------------------------------------------------------------ relative positions, float64 from the table's angles
def _rot(x, a):
    """x float64 [hd] rotated by the angles a float64 [hd / 2]"""
    p = x.reshape(-1, 2)
    return np.stack([p[:, 0] * np.cos(a) - p[:, 1] * np.sin(a), p[:, 0] * np.sin(a) + p[:, 1] * np.cos(a)], -1).reshape(-1)


@pytest.mark.parametrize("hd", [64, 128])
def test_1d_scores_depend_on_the_offset_only(hd):
    T, P = 16, 256
    a = ro.rotary_angles("1d", T, P, hd)
    rng = np.random.default_rng(hd)
    for i, j, t in ((0, 0, 5), (3, 1, 100), (40, 7, 200), (200, 150, 71), (T + 5, 2, 33)):
        q, k = rng.standard_normal(hd), rng.standard_normal(hd)
        s0 = _rot(q, a[i]) @ _rot(k, a[j])
        s1 = _rot(q, a[i + t]) @ _rot(k, a[j + t])
        assert abs(s0 - s1) <= 1e-10 * (np.linalg.norm(q) * np.linalg.norm(k)), (i, j, t, s0, s1)


@pytest.mark.parametrize("hd", [64, 128])
def test_axial_scores_depend_on_the_grid_offset_only(hd):
    """two image tokens moved by the same (row, column) offset keep their score; moving one of them alone changes it by many
    orders of magnitude more"""
    T, P, G = 16, 256, 16
    a = ro.rotary_angles("axial", T, P, hd)
    rng = np.random.default_rng(hd + 1)
    at = lambda r, c: T + r * G + c    # noqa: E731
    worst_same, least_single = 0.0, np.inf
    for (ri, ci), (rj, cj), (dr, dc) in (((0, 0), (0, 0), (3, 4)), ((5, 2), (1, 9), (7, 3)), ((10, 10), (2, 3), (5, -3)),
                                         ((4, 15), (4, 0), (-4, 0)), ((9, 1), (8, 14), (6, 1))):
        q, k = rng.standard_normal(hd), rng.standard_normal(hd)
        scale = np.linalg.norm(q) * np.linalg.norm(k)
        s0 = _rot(q, a[at(ri, ci)]) @ _rot(k, a[at(rj, cj)])
        both = _rot(q, a[at(ri + dr, ci + dc)]) @ _rot(k, a[at(rj + dr, cj + dc)])
        single = _rot(q, a[at(ri + dr, ci + dc)]) @ _rot(k, a[at(rj, cj)])
        worst_same = max(worst_same, abs(both - s0) / scale)
        least_single = min(least_single, abs(single - s0) / scale)
    assert worst_same <= 1e-12, worst_same
    assert least_single >= 1e6 * max(worst_same, 1e-16), (least_single, worst_same)
    # a flat shift by t (which wraps rows) is NOT a grid offset: the axial scheme does not keep it
    q, k = rng.standard_normal(hd), rng.standard_normal(hd)
    s0 = _rot(q, a[at(3, 12)]) @ _rot(k, a[at(1, 2)])
    s1 = _rot(q, a[at(3, 12) + 7]) @ _rot(k, a[at(1, 2) + 7])
    assert abs(s1 - s0) >= 1e6 * max(worst_same, 1e-16) * np.linalg.norm(q) * np.linalg.norm(k)


# ------------------------------------------------------------------ ABI
def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_entry_points_are_declared_exported_and_bound():
    raw = ctypes.CDLL(dh.LIB_PATH)
    for name, nargs in (("dmi_rope_qk", 9), ("dmi_rope_qk_decode", 9)):
        assert name in dh.declared_symbols(), name
        assert hasattr(raw, name), name
        fn = getattr(dh.lib(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
        assert callable(getattr(dh, name[4:]))
    assert dh.lib().dmi_rope_qk.argtypes[3] is ctypes.c_int64        # the row count travels whole


def test_refusals_come_before_any_launch():
    L = dh.lib()
    qk = lambda qkv=A, ld=768, cs=C, rows=8, S=4, H=2, hd=128: L.dmi_rope_qk(qkv, ld, cs, rows, S, H, hd, 0, None)   # noqa: E731
    dec = lambda fresh=A, cs=C, B=2, S=4, H=2, hd=128, pos=0, pos_dev=None: L.dmi_rope_qk_decode(fresh, cs, B, S, H, hd, pos, pos_dev, None)   # noqa: E731
    for call, prefix, ptrs in ((qk, "rope_qk:", ("qkv", "cs")), (dec, "rope_qk_decode:", ("fresh", "cs"))):
        for p in ptrs:
            assert call(**{p: None}) == INVALID and _msg().startswith(prefix) and "null" in _msg(), (p, _msg())
            assert call(**{p: A + 8}) == INVALID and _msg().startswith(prefix) and "aligned" in _msg(), (p, _msg())
        for hd in (32, 96, 256, 0):
            assert call(hd=hd) == UNSUPPORTED and _msg().startswith(prefix) and "64 or 128" in _msg(), (hd, _msg())
        assert call(H=0) == INVALID and _msg().startswith(prefix)
        assert call(S=0) == INVALID and _msg().startswith(prefix)
    assert qk(rows=0) == INVALID and qk(rows=-4) == INVALID
    assert qk(ld=500) == INVALID and "ld" in _msg()        # narrower than q | k
    assert qk(ld=516) == INVALID and "ld" in _msg()        # rows would lose their 16-byte alignment
    assert dec(B=0) == INVALID
    for pos in (-1, 4, 1 << 20):
        assert dec(pos=pos) == INVALID and "pos" in _msg(), (pos, _msg())


# ------------------------------------------------------------------ the rotated oracle
def test_zero_angle_table_reproduces_the_plain_oracle_exactly():
    from oracle import dalle_oracle as do
    T, P, TV, IV = 8, 16, 50, 16
    cfg = do.DalleConfig(64, TV, IV, T, P, 2, 2)
    P0 = do.init_params(cfg, seed=5, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(2, T, TV, seed=1), do.synthetic_image_tokens(2, P, IV, seed=2), TV)
    table = np.zeros((T + P, cfg.kv_dim // 2, 2), np.float32)
    table[..., 0] = 1.0
    loss_r, g_r = sref.loss_and_grads(P0, tokens, cfg, table=table)
    loss_o, g_o = do.loss_and_grads(P0, tokens, cfg)
    assert loss_r == loss_o
    for k in g_o:
        assert np.array_equal(g_r[k], g_o[k]), k
    # and a real table moves the q / k gradients
    loss_x, g_x = sref.loss_and_grads(P0, tokens, cfg, table=ro.rotary_table("axial", T, P, cfg.kv_dim))
    assert loss_x != loss_o and not np.array_equal(g_x["layer_0/attn/q"], g_o["layer_0/attn/q"])


def test_rope64_matches_the_differentiable_rotation_and_inverts():
    import torch
    rng = np.random.default_rng(3)
    S, H, hd, B = 24, 2, 64, 2
    cs = ro.rotary_table("1d", 8, 16, hd)
    x = rng.standard_normal((B * S, 3 * H * hd))
    y = rref.rope64(x, cs, H, hd, S)
    assert np.array_equal(y[:, 2 * H * hd:], x[:, 2 * H * hd:])
    q = torch.from_numpy(x[:, :H * hd].reshape(B, S, H, hd).transpose(0, 2, 1, 3).copy())
    yq = rref.rotate(q, torch.from_numpy(cs.astype(np.float64))).numpy().transpose(0, 2, 1, 3).reshape(B * S, H * hd)
    assert np.abs(yq - y[:, :H * hd]).max() <= 1e-14
    back = rref.rope64(y, cs, H, hd, S, inverse=True)
    assert np.abs(back - x).max() <= 1e-6        # the table is float32: cos^2 + sin^2 = 1 to its rounding
