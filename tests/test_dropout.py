"""Embedding / residual dropout on the CPU: the ABI of the four dropout entry points and their refusals, the config keys, the mask's
statistics and keys, the masked oracle's distance from the plain one, and the new kernels' compile-time resources."""
import ctypes
import math
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))

import dalle_hip as dh  # noqa: E402
import dalle_step_ref as sref  # noqa: E402
import dropout_ref as dref  # noqa: E402
from engine_case import BATCH, NL, P, T, inputs  # noqa: E402
from parity import rel_l2  # noqa: E402
from src.dalle_mtf import dropout as dr  # noqa: E402

# the engine-step tests here (the masks matter) and in tests/test_dropout_gpu.py: the shared case at both widths (n_embd 512 is where the
# fused LayerNorm products would otherwise run)
RATE = 0.25
WIDTHS = [(256, 2), (512, 4)]

SYMBOLS = {"dmi_dropout_add_ln": 14, "dmi_dropout_bwd": 7, "dmi_embed_fwd_dropout": 12, "dmi_embed_bwd_dropout": 14}
A, B, C, D = 0x10000, 0x20000, 0x30000, 0x40000     # fake device pointers: every refusal comes before a launch, none is dereferenced
INVALID = -1


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_entry_points_are_declared_exported_and_bound():
    raw = ctypes.CDLL(dh.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert name in dh.declared_symbols(), name
        assert hasattr(raw, name), name
        fn = getattr(dh.lib(), name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name
        assert ctypes.c_uint64 in fn.argtypes, name           # the 64-bit key travels whole
        assert callable(getattr(dh, name[4:]))


def _add_ln(a=A, res=B, x=C, g=D, b=D, y=A, mean=B, rstd=C, M=4, d=128, thresh=100):
    return dh.lib().dmi_dropout_add_ln(a, res, x, g, b, y, mean, rstd, M, d, 7, thresh, 1e-5, None)


def _bwd(dx=A, dy=B, M=4, d=128, thresh=100):
    return dh.lib().dmi_dropout_bwd(dx, dy, M, d, 7, thresh, None)


def _efwd(tok=A, wte=B, wpe=C, x=D, rows=8, S=4, d=128, thresh=100):
    return dh.lib().dmi_embed_fwd_dropout(tok, wte, wpe, x, rows, S, d, 50, 7, 8, thresh, None)


def _ebwd(st=A, perm=B, dx=C, dwte=D, dwpe=A, Bn=2, S=4, d=128, ws=B, thresh=100):
    return dh.lib().dmi_embed_bwd_dropout(st, perm, dx, dwte, dwpe, Bn, S, d, 50, ws, 7, 8, thresh, None)


def test_refusals_come_before_any_launch():
    for call, prefix, ptrs, rows in ((_add_ln, "dropout_add_ln", ("a", "res", "x"), "M"), (_bwd, "dropout_bwd", ("dx", "dy"), "M"),
                                     (_efwd, "embed_fwd_dropout", ("tok", "wte", "wpe", "x"), "rows"),
                                     (_ebwd, "embed_bwd_dropout", ("st", "perm", "dx", "dwte", "dwpe", "ws"), "Bn")):
        for p in ptrs:
            assert call(**{p: None}) == INVALID, (prefix, p)
            assert _msg().startswith(prefix) and "null" in _msg(), _msg()
        for d in (12, 100, 4):
            assert call(d=d) == INVALID and _msg().startswith(prefix) and "% 8" in _msg(), (prefix, d, _msg())
        for m in (0, -3):
            assert call(**{rows: m}) == INVALID and _msg().startswith(prefix), (prefix, m)
        for t in (-1, 65536, 1 << 20):
            assert call(thresh=t) == INVALID and "thresh" in _msg() and "65535" in _msg(), (prefix, t, _msg())
        with pytest.raises(dh.DalleHipError, match="thresh"):
            dh._check(call(thresh=-5), prefix)
    # the LayerNorm half's pointers are needed only with gamma; d is bounded by the row-in-registers LayerNorm
    for p in ("b", "y", "mean", "rstd"):
        assert _add_ln(**{p: None}) == INVALID and "null" in _msg(), p
    assert _add_ln(d=4104) == INVALID and "4096" in _msg()
    assert _add_ln(a=A + 8) == INVALID and "16-byte aligned" in _msg()
    assert _bwd(dy=B + 2) == INVALID and "16-byte aligned" in _msg()


def test_config_keys():
    assert dr.resolve_dropout(None) == (0, 0, 0) and dr.resolve_dropout({}) == (0, 0, 0)
    assert dr.resolve_dropout({"embed_dropout": None, "residual_dropout": 0, "dropout_seed": None}) == (0, 0, 0)
    assert dr.resolve_dropout({"embed_dropout": 0.1, "residual_dropout": 0.5, "dropout_seed": 9}) == (6554, 32768, 9)
    assert dr.resolve_dropout({"residual_dropout": 0.25}) == (0, 16384, 0)
    assert dr.resolve_dropout({"embed_dropout": 0.9999999}) == (65535, 0, 0)        # clamped: scale stays finite
    for k in dr.KEYS:
        for bad in (-0.1, 1.0, 1, float("nan"), float("inf"), "0.1", True, 1.5):
            with pytest.raises(ValueError, match=k):
                dr.resolve_dropout({k: bad})
    for bad in (0.5, "3", True):
        with pytest.raises(ValueError, match="dropout_seed"):
            dr.resolve_dropout({"dropout_seed": bad})


def test_constructor_checks_the_keys_before_any_device_work():
    """no GPU here: a constructor that reached the engine would raise DalleHipError instead"""
    from src.dalle_mtf.models import DALLE
    for k in ("embed_dropout", "residual_dropout"):
        for bad in (-0.1, 1.0, float("nan"), "0.1"):
            with pytest.raises(ValueError, match=k):
                DALLE(256, n_heads=2, params={k: bad})
    with pytest.raises(NotImplementedError, match="attention_dropout.*embed_dropout and residual_dropout are"):
        DALLE(256, n_heads=2, params={"attention_dropout": 0.1})
    with pytest.raises(NotImplementedError, match="attention_dropout"):
        DALLE(256, n_heads=2, params={"attention_dropout": 0.1, "residual_dropout": 0.1})
    # the untouched refusals still come first or alike
    with pytest.raises(NotImplementedError, match="loss_fn"):
        DALLE(256, n_heads=2, loss_fn=lambda *a: 0, params={"residual_dropout": 0.1})
    with pytest.raises(NotImplementedError, match="scale_type"):
        DALLE(256, n_heads=2, params={"residual_dropout": 0.1, "scale_type": "other"})


def test_shipped_configs_leave_dropout_off():
    from src.utils import fetch_model_params
    for name in ("dalle_example", "dalle_coco"):
        assert dr.resolve_dropout(fetch_model_params(os.path.join(ROOT, "configs", name + ".json")))[:2] == (0, 0), name


def test_host_module_and_numpy_restatement_agree():
    for x in (0, 1, 0xdeadbeef, (1 << 64) - 1, 0x9E3779B97F4A7C15):
        assert dr.splitmix64(x) == int(dref.splitmix64(np.uint64(x)))
    assert dr.splitmix64(0) == 0xE220A8397B1DCDAF        # the published first output of the generator seeded with 0
    for args in ((0, 0, 0, 0, 0), (1234, 3000, 3, 7, 13), ((1 << 63) + 5, 10 ** 9, 0, 255, 2)):
        assert dr.site_key(*args) == dref.site_key(*args)
    for rate in (0.0, 0.1, 0.25, 0.5, 1e-6, 0.99999):
        t = dr.threshold(rate)
        assert t == dref.threshold(rate) and 0 <= t <= 65535
        assert dr.scale(t) == dref.scale(t) and dr.scale(t).dtype == np.float32
    assert (dr.SITE_TOKEN, dr.SITE_POSITION, dr.site_attention(0), dr.site_mlp(0), dr.site_attention(4), dr.site_mlp(4)) == (0, 1, 2, 3, 10, 11)


@pytest.mark.parametrize("rate", [0.1, 0.5])
def test_kept_fraction_is_binomial(rate):
    n = 1 << 20
    t = dref.threshold(rate)
    p = 1.0 - t / 65536.0
    kept = int(dref.keep(dref.site_key(0, 0, 0, 0, 2), t, n).sum())
    assert abs(kept - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p)), (kept, n * p)
    # expectation: keep probability times scale is 1 up to fp32 rounding of the scale
    assert abs(p * float(dref.scale(t)) - 1.0) < 1e-6


def test_threshold_zero_keeps_everything_at_scale_one():
    assert dref.threshold(0.0) == 0 and dref.scale(0) == np.float32(1.0) and dr.scale(0) == np.float32(1.0)
    assert dref.keep(12345, 0, 4096).all()
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    assert np.array_equal(dref.drop(x, 12345, 0), x)


def test_keys_are_pairwise_distinct():
    L = 6
    keys = [dr.site_key(0, step, mb, rank, site) for step in range(4) for mb in range(3) for rank in range(3) for site in range(2 + 2 * L)]
    assert len(set(keys)) == len(keys)
    assert dr.site_key(1, 0, 0, 0, 0) != dr.site_key(0, 0, 0, 0, 0)
    # the masks of two keys differ (not just the keys)
    a, b = dref.keep(keys[0], 16384, 4096), dref.keep(keys[1], 16384, 4096)
    assert 0.2 < float((a != b).mean()) < 0.6


@pytest.mark.parametrize("n_embd,n_heads", WIDTHS)
def test_masked_oracle_is_far_from_the_plain_one(n_embd, n_heads):
    """fp32 only: at rate 0.25, dropout_seed 0, step 0 the masks move some gradient tensor by more than 0.2 relative L2 -- what the
    GPU test then asserts of the engine"""
    cfg, P0, tokens = inputs(n_embd, n_heads)
    t = dref.threshold(RATE)
    last = {site: (dref.site_key(0, 0, 0, 0, site), t) for site in range(2 + 2 * NL)}
    masks = dref.engine_masks(last, BATCH, T + P, n_embd, NL)
    loss_m, gm = sref.loss_and_grads(P0, tokens, cfg, dropout=masks)
    loss_p, gp = sref.loss_and_grads(P0, tokens, cfg)
    from oracle import dalle_oracle as do
    loss_o, go = do.loss_and_grads(P0, tokens, cfg)
    assert abs(loss_p - loss_o) <= 1e-6 * abs(loss_o) and max(rel_l2(gp[k], go[k]) for k in go) < 1e-5     # the composition is the oracle's
    worst = max(rel_l2(gm[k], gp[k]) for k in gp)
    print("masked vs plain fp32 oracle: loss", loss_m, loss_p, "worst grad rel L2", worst)
    assert worst > 0.2, worst


def test_new_kernels_use_no_scratch_and_do_not_spill():
    from dalle_hip import build as b
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([b._hipcc()] + b.FLAGS + ["-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(ROOT, "dalle-mtf_amd", "csrc", "elementwise.hip"), "-o", os.path.join(tmp, "e.o")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    usage = {}
    for blk in re.split(r"remark: Function Name: ", p.stdout)[1:]:
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))   # noqa: E731
        usage[blk.split()[0]] = dict(scratch=g(r"ScratchSize \[bytes/lane\]"), sgpr_spill=g("SGPRs Spill"), vgpr_spill=g("VGPRs Spill"),
                                     occupancy=g(r"Occupancy \[waves/SIMD\]"))
    # dropout_add_ln <1 | 2 | 4 | 8>, dropout_bwd, and the DROP = true instances of the three embedding kernels (ILb1E in the symbol)
    mine = {k: v for k, v in usage.items() if "dropout_add_ln_kernel" in k or "dropout_bwd_kernel" in k
            or (("embed_fwd_kernel" in k or "embed_bwd_wpe_kernel" in k or "embed_bwd_wte_sorted_kernel" in k) and "ILb1E" in k)}
    assert len(mine) == 8, sorted(mine)
    for k, u in mine.items():
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (k, u)
