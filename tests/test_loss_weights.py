"""Text/image loss weights on the CPU (config keys "text_loss_weight" / "image_loss_weight", DESIGN.md §4 "Loss weights"): the
position-weight builder, the refusals, the float64 helper tests/loss_weights_ref.py, and the two new C entry points (declared,
exported, bound; argument errors come back as a status before anything is launched -- the pointers are never dereferenced)."""
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
from loss_weights_ref import loss_reduce_ref, position_weights_ref, weighted_loss_ref  # noqa: E402
from src.dalle_mtf.loss_weights import KEYS, position_weights, resolve_loss_weights  # noqa: E402

FAKE = ctypes.c_void_p(0x10000)
DMI_ERR_INVALID = -1


@pytest.mark.parametrize("T,P,wt,wi", [(16, 112, 1, 7), (256, 1024, 1, 7), (2, 6, 3.5, 0.25), (24, 40, 0, 1), (24, 40, 1, 0),
                                       (77, 1, 1e-3, 1e3)])
def test_position_weights_sum_to_one_and_match_the_restatement(T, P, wt, wi):
    w = position_weights(T, P, wt, wi)
    assert w.dtype == np.float64 and w.shape == (T + P,)
    assert abs(w.sum() - 1.0) <= 1e-14
    assert np.array_equal(w, position_weights_ref(T, P, wt, wi))
    assert len(set(w[:T - 1])) == 1 and len(set(w[T - 1:])) == 1     # one value per modality, the boundary at p = T - 1


def test_weights_in_the_ratio_of_the_position_counts_are_uniform():
    """wt : wi = (T - 1) : (P + 1) gives 1 / S everywhere, exactly when S is a power of two"""
    w = position_weights(16, 112, 15, 113)
    assert np.all(w == 1.0 / 128)
    assert np.all(w.astype(np.float32) == np.float32(1.0 / 128))


def test_a_zero_weight_zeroes_that_modality():
    w = position_weights(16, 112, 1, 0)
    assert np.all(w[15:] == 0.0) and np.all(w[:15] == 1.0 / 15)
    w = position_weights(16, 112, 0, 1)
    assert np.all(w[:15] == 0.0) and np.all(w[15:] == 1.0 / 113)


def test_resolution_either_key_alone_implies_one_for_the_other():
    assert KEYS == ("text_loss_weight", "image_loss_weight")
    assert resolve_loss_weights({}, 16) is None and resolve_loss_weights(None, 16) is None
    assert resolve_loss_weights({"text_loss_weight": None, "image_loss_weight": None}, 1) is None     # unset: nothing to check
    assert resolve_loss_weights({"image_loss_weight": 7}, 16) == (1.0, 7.0)
    assert resolve_loss_weights({"text_loss_weight": 0.5}, 16) == (0.5, 1.0)
    assert resolve_loss_weights({"text_loss_weight": 1, "image_loss_weight": 7}, 2) == (1.0, 7.0)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("bad", [-1, -1e-9, float("nan"), float("inf"), float("-inf"), "7", True])
def test_bad_values_are_refused_naming_the_key(key, bad):
    with pytest.raises(ValueError, match=key):
        resolve_loss_weights({key: bad}, 16)


def test_both_zero_and_a_one_token_caption_are_refused():
    with pytest.raises(ValueError, match="text_loss_weight.*image_loss_weight"):
        resolve_loss_weights({"text_loss_weight": 0, "image_loss_weight": 0.0}, 16)
    with pytest.raises(ValueError, match="text_loss_weight.*text_seq_len"):
        resolve_loss_weights({"image_loss_weight": 7}, 1)


def test_constructors_refuse_before_any_device_work():
    """the checks run before the engine looks for a GPU, so they hold on a machine without one"""
    from src.dalle_mtf.engine import DalleEngine
    from src.dalle_mtf.models import DALLE
    with pytest.raises(ValueError, match="image_loss_weight"):
        DALLE(256, n_heads=2, params={"image_loss_weight": -7})
    with pytest.raises(ValueError, match="text_loss_weight"):
        DALLE(256, n_heads=2, params={"text_loss_weight": float("nan"), "image_loss_weight": 7})
    with pytest.raises(ValueError, match="text_seq_len"):
        DALLE(256, n_heads=2, text_seq_len=1, image_seq_len=7, params={"text_loss_weight": 1})
    with pytest.raises(ValueError, match="image_loss_weight"):
        DalleEngine(256, 2, 2, 300, 64, 16, 112, batch_size=2, hparams={"text_loss_weight": 0, "image_loss_weight": 0})


def test_reference_helper_reproduces_the_formula_and_the_static_weights():
    rng = np.random.default_rng(5)
    for T, P, wt, wi in [(16, 112, 1, 7), (5, 11, 2.5, 0.5), (3, 4, 0, 1)]:
        lb = rng.uniform(0.1, 9.0, size=(6, T + P))
        loss, mt, mi = weighted_loss_ref(lb, T, wt, wi)
        assert mt == lb[:, :T - 1].mean() and mi == lb[:, T - 1:].mean()
        assert abs(loss - (wt * mt + wi * mi) / (wt + wi)) <= 1e-15 * loss
        # the same number from the static position weights: 1 / B * sum_{b,p} w[p] NLL[b,p]
        assert abs(loss - (lb * position_weights(T, P, wt, wi)[None]).sum() / 6) <= 1e-13 * loss
        three = loss_reduce_ref(lb.ravel(), position_weights(T, P, wt, wi), T - 1, 1.0 / 6)
        assert np.allclose(three, [loss, mt, mi], rtol=1e-13, atol=0)


def test_loss_weight_entry_points_are_declared_exported_and_bound():
    L = dh.lib()
    declared = dh.declared_symbols()
    for name in ("dmi_softmax_finish_w", "dmi_loss_reduce"):
        assert name in declared, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert len(L.dmi_softmax_finish_w.argtypes) == len(L.dmi_softmax_finish.argtypes) + 2
    assert len(L.dmi_loss_reduce.argtypes) == 8
    assert callable(dh.softmax_finish_w) and callable(dh.loss_reduce)


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_argument_checks_of_the_two_entry_points():
    L = dh.lib()
    p = FAKE

    def finish_w(pos_weight, period):
        return L.dmi_softmax_finish_w(p, 8, p, None, p, p, 128, p, 128, p, p, 1024, 1024, p, p, p, p, p, 111, 128, 1000, 0.5,
                                      pos_weight, period, None)
    assert finish_w(None, 37) == DMI_ERR_INVALID and _msg().startswith("softmax_finish_w") and "null" in _msg()
    assert finish_w(p, 0) == DMI_ERR_INVALID and "period" in _msg()
    assert finish_w(p, -3) == DMI_ERR_INVALID and "period" in _msg()
    for args in ((None, 10, p, 4, 2, 1.0, p), (p, 10, None, 4, 2, 1.0, p), (p, 10, p, 4, 2, 1.0, None)):
        assert L.dmi_loss_reduce(*args, None) == DMI_ERR_INVALID and _msg().startswith("loss_reduce") and "null" in _msg()
    for M, period, split in ((0, 4, 2), (10, 0, 0), (10, 4, -1), (10, 4, 5)):
        assert L.dmi_loss_reduce(p, M, p, period, split, 1.0, p, None) == DMI_ERR_INVALID and "period" in _msg()
