"""Padded caption positions in the loss, the config key "loss_ignore_padding" (DESIGN.md §4 "Loss: padded caption positions"):
the host side -- resolution of the key, the float64 row weights against the independent restatement of tests/loss_mask_ref.py, the
equivalence with the plain and the weighted loss when nothing is padded -- and the C ABI's argument checks.  CPU only."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
import dalle_hip as dh  # noqa: E402
from loss_mask_ref import keep_ref, masked_loss_ref, out4_ref, row_weights_ref  # noqa: E402
from loss_weights_ref import weighted_loss_ref  # noqa: E402
from src.dalle_mtf.loss_mask import KEY, mask_coefficients, resolve_loss_ignore_padding, row_weights  # noqa: E402

FAKE = ctypes.c_void_p(0x10000)
DMI_ERR_INVALID = -1


# ------------------------------------------------------------------ the key
def test_off_forms():
    assert KEY == "loss_ignore_padding"
    for params in (None, {}, {KEY: None}, {KEY: False}):
        assert resolve_loss_ignore_padding(params, 16, 300) == (False, None)
    # off: nothing else is looked at
    assert resolve_loss_ignore_padding({KEY: False, "padding_id": -5}, 1, 300) == (False, None)


@pytest.mark.parametrize("bad", [1, 0, "true", "yes", 1.0, [True], np.bool_(True)])
def test_only_a_bool_is_accepted(bad):
    with pytest.raises(ValueError, match=KEY):
        resolve_loss_ignore_padding({KEY: bad}, 16, 300)


def test_padding_id_and_its_fallback():
    assert resolve_loss_ignore_padding({KEY: True}, 16, 300) == (True, 299)
    assert resolve_loss_ignore_padding({KEY: True, "padding_id": None}, 16, 300) == (True, 299)
    assert resolve_loss_ignore_padding({KEY: True, "padding_id": 0}, 16, 300) == (True, 0)
    assert resolve_loss_ignore_padding({KEY: True, "padding_id": np.int64(57)}, 2, 300) == (True, 57)


@pytest.mark.parametrize("pad", [-1, 300, 50257, 3.0, "299", True])
def test_padding_id_outside_the_text_vocabulary_is_refused(pad):
    with pytest.raises(ValueError, match=KEY):
        resolve_loss_ignore_padding({KEY: True, "padding_id": pad}, 16, 300)


def test_a_one_token_caption_is_refused():
    with pytest.raises(ValueError, match=KEY + ".*text_seq_len"):
        resolve_loss_ignore_padding({KEY: True}, 1, 300)


def test_constructors_refuse_before_any_device_work():
    """the checks run before the engine looks for a GPU, so they hold on a machine without one"""
    from src.dalle_mtf.engine import DalleEngine
    from src.dalle_mtf.models import DALLE
    with pytest.raises(ValueError, match=KEY):
        DALLE(256, n_heads=2, params={KEY: 1})
    with pytest.raises(ValueError, match=KEY):
        DALLE(256, n_heads=2, text_vocab_size=300, params={KEY: True, "padding_id": 300})
    with pytest.raises(ValueError, match="text_seq_len"):
        DALLE(256, n_heads=2, text_seq_len=1, image_seq_len=7, params={KEY: True})
    with pytest.raises(ValueError, match=KEY):
        DalleEngine(256, 2, 2, 300, 64, 16, 112, batch_size=2, hparams={KEY: "on"})
    # the options' errors come first, in their own order
    with pytest.raises(ValueError, match="image_loss_weight"):
        DALLE(256, n_heads=2, params={KEY: 1, "image_loss_weight": -7})


def test_the_key_is_not_a_field_of_options():
    from src.dalle_mtf.options import Options, checkpoint_entries, report, resolve_options
    assert KEY not in Options._fields
    opt = resolve_options({KEY: True}, 256, 16, 256)
    assert KEY not in checkpoint_entries(opt) and KEY not in report(opt)


# ------------------------------------------------------------------ the formulas
def _labels(B, T, P, pad, rng, lengths=None):
    """labels [B, T + P] of right-padded captions (label p = token p + 1): text labels below pad, image labels at or above pad + 1"""
    lab = np.empty((B, T + P), np.int64)
    for b in range(B):
        n = int(rng.integers(1, T + 1)) if lengths is None else lengths[b]
        tok = np.full(T, pad)
        tok[:n] = rng.integers(0, pad, size=n)
        lab[b, :T - 1] = tok[1:]
        lab[b, T - 1:] = rng.integers(pad + 1, pad + 65, size=P + 1)
    return lab


@pytest.mark.parametrize("weights", [None, (1, 7), (2.5, 0.5), (0, 1), (1, 0)])
@pytest.mark.parametrize("lengths", [None, [1, 1, 1], [9, 9, 9]], ids=["random", "all-padded", "none-padded"])
def test_row_weights_match_the_restatement(weights, lengths):
    T, P, pad = 9, 14, 40
    lab = _labels(3, T, P, pad, np.random.default_rng(3), lengths)
    c, n_t, n_i = row_weights(lab, T, pad, weights)
    keep, nt, ni = keep_ref(lab, T - 1, pad)
    assert (n_t, n_i) == (nt, ni) and n_i == 3 * (P + 1)
    if lengths is not None:
        assert n_t == (0 if lengths[0] == 1 else 3 * (T - 1))
    ref = row_weights_ref(lab, T - 1, pad, weights)
    assert c.dtype == np.float64 and np.all(np.abs(c - ref) <= 1e-15 * np.abs(ref))
    assert np.all(c[~keep] == 0.0)
    if weights is None:
        assert abs(c.sum() - 1.0) <= 1e-14
    else:      # the text rows carry ct (0 when none is kept: nothing is renormalised), the image rows ci
        ct, ci, plain = mask_coefficients(weights)
        assert not plain and abs(ct + ci - 1.0) <= 1e-15
        assert abs(c[:, :T - 1].sum() - (ct if n_t else 0.0)) <= 1e-14 and abs(c[:, T - 1:].sum() - ci) <= 1e-14


@pytest.mark.parametrize("weights", [None, (1, 7), (2.5, 0.5)])
def test_masked_loss_is_sum_c_nll_and_its_parts(weights):
    T, P, pad = 9, 14, 40
    rng = np.random.default_rng(11)
    lab = _labels(4, T, P, pad, rng)
    lb = rng.uniform(0.1, 9.0, size=lab.shape)
    loss, lt, li, frac = masked_loss_ref(lb, lab, T, pad, weights)
    c, n_t, n_i = row_weights(lab, T, pad, weights)
    assert 0 < n_t < 4 * (T - 1)
    assert abs((c * lb).sum() - loss) <= 1e-13 * loss
    o4 = out4_ref(lb, lab, T - 1, pad, weights, 0.5)
    assert np.all(np.abs(o4 - np.array([0.5 * loss, lt, li, frac])) <= 1e-13 * np.abs(o4))
    assert frac == n_t / (4 * (T - 1))


@pytest.mark.parametrize("weights", [None, (1, 7), (0, 1)])
def test_with_no_padded_label_the_masked_loss_is_the_plain_or_weighted_loss(weights):
    T, P, pad = 9, 14, 40
    rng = np.random.default_rng(5)
    lab = _labels(3, T, P, pad, rng, lengths=[T, T, T])
    lb = rng.uniform(0.1, 9.0, size=lab.shape)
    loss, lt, li, frac = masked_loss_ref(lb, lab, T, pad, weights)
    ref, mt, mi = (lb.mean(), lb[:, :T - 1].mean(), lb[:, T - 1:].mean()) if weights is None else weighted_loss_ref(lb, T, *weights)
    assert frac == 1.0
    assert abs(loss - ref) <= 1e-14 * ref and abs(lt - mt) <= 1e-14 * mt and abs(li - mi) <= 1e-14 * mi
    c, _, _ = row_weights(lab, T, pad, weights)
    assert abs((c * lb).sum() - ref) <= 1e-13 * ref


def test_an_all_padded_batch_keeps_the_image_term_unrenormalised():
    T, P, pad = 9, 14, 40
    rng = np.random.default_rng(6)
    lab = _labels(2, T, P, pad, rng, lengths=[1, 1])
    lb = rng.uniform(0.1, 9.0, size=lab.shape)
    loss, lt, li, frac = masked_loss_ref(lb, lab, T, pad, (1, 7))
    assert lt == 0.0 and frac == 0.0 and abs(loss - 7 / 8 * li) <= 1e-15
    c, n_t, _ = row_weights(lab, T, pad, (1, 7))
    assert n_t == 0 and np.all(c[:, :T - 1] == 0.0) and abs((c * lb).sum() - 7 / 8 * li) <= 1e-14


# ------------------------------------------------------------------ the C ABI
def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_entry_points_are_declared_exported_and_bound():
    L = dh.lib()
    declared = dh.declared_symbols()
    for name, n in (("dmi_loss_mask", 11), ("dmi_loss_reduce_masked", 11)):
        assert name in declared, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == n and fn.restype is ctypes.c_int, name
    assert callable(dh.loss_mask) and callable(dh.loss_reduce_masked)


def test_argument_checks_refuse_before_a_launch():
    L = dh.lib()
    p = FAKE
    for args in ((None, 10, 4, 2, 3, 0.5, 0.5, 0, p, p), (p, 10, 4, 2, 3, 0.5, 0.5, 0, None, p), (p, 10, 4, 2, 3, 0.5, 0.5, 0, p, None)):
        assert L.dmi_loss_mask(*args, None) == DMI_ERR_INVALID and _msg().startswith("loss_mask") and "null" in _msg()
    for M, period, split in ((10, 0, 0), (10, -4, 0), (10, 4, -1), (10, 4, 5)):
        assert L.dmi_loss_mask(p, M, period, split, 3, 0.5, 0.5, 0, p, p, None) == DMI_ERR_INVALID and "period" in _msg()
    for M in (0, 1 << 31):
        assert L.dmi_loss_mask(p, M, 4, 2, 3, 0.5, 0.5, 0, p, p, None) == DMI_ERR_INVALID and "M" in _msg()
    ok = (p, p, p, 10, 4, 2, 3, p, 1.0, p)
    for i in (0, 1, 2, 7, 9):
        args = list(ok)
        args[i] = None
        assert L.dmi_loss_reduce_masked(*args, None) == DMI_ERR_INVALID and _msg().startswith("loss_reduce_masked") and "null" in _msg()
    for M, period, split in ((0, 4, 2), (10, 0, 0), (10, 4, -1), (10, 4, 5)):
        assert L.dmi_loss_reduce_masked(p, p, p, M, period, split, 3, p, 1.0, p, None) == DMI_ERR_INVALID and "period" in _msg()
