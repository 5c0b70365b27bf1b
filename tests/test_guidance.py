"""Classifier-free guidance, CPU side: the guided-draw C ABI (declared, exported, bound; argument errors come back as a status and
a message before anything is launched -- the pointers below are never dereferenced), the restated guided logits on hand-built
rows, generate_dalle.py's argument checks, and the "caption_dropout" key of the input pipeline."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dalle_hip as dh  # noqa: E402
from guidance_ref import guided_keep, guided_logits  # noqa: E402

FAKE = ctypes.c_void_p(0x10000)
DMI_ERR_INVALID = -1


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def _call(z=FAKE, Bc=2, nv=64, top_p=0.9, scale=3.0, advance=0, pos_dev=None, next_tok=FAKE, out=None):
    return dh.lib().dmi_sample_tokens_guided(z, nv, None, Bc, nv, 1.0, 0, 0, top_p, scale, None, 0, pos_dev, advance, 0, next_tok, out,
                                             0, 0, None, None)


def test_guided_entry_point_is_declared_exported_and_bound():
    L = dh.lib()
    assert "dmi_sample_tokens_guided" in dh.declared_symbols()
    fn = L.dmi_sample_tokens_guided
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 21
    assert len(L.dmi_sample_tokens_p.argtypes) == 20 and len(L.dmi_sample_tokens.argtypes) == 18    # the others keep their signatures
    assert callable(dh.sample_tokens_guided)
    bits = lambda x: int(np.array([x], np.float32).view(np.uint32)[0])   # noqa: E731
    prm = dh.sample_params(0.5, 7, (3 << 32) | 9, top_p=0.25, guidance_scale=3.0)
    assert prm.shape == (6,) and prm.numpy().view(np.uint32).tolist() == [bits(2.0), 7, 9, 3, bits(0.25), bits(3.0)]
    # without the new keyword the helper returns the words it always returned
    assert dh.sample_params(0.5, 7, (3 << 32) | 9, top_p=0.25).numpy().view(np.uint32).tolist() == [bits(2.0), 7, 9, 3, bits(0.25), 0]
    assert dh.sample_params(0.5, 7, 9).shape == (4,)


@pytest.mark.parametrize("scale", [-0.5, -1e-30, float("nan"), float("inf"), float("-inf")])
def test_a_negative_or_non_finite_scale_is_refused(scale):
    assert _call(scale=scale) == DMI_ERR_INVALID
    msg = _msg()
    assert msg.startswith("sample_tokens_guided") and "scale" in msg, msg
    with pytest.raises(dh.DalleHipError):
        dh._check(_call(scale=scale), "sample_tokens_guided")


@pytest.mark.parametrize("top_p", [0.0, -0.1, 1.5, float("nan"), float("inf")])
def test_top_p_outside_the_unit_interval_is_refused(top_p):
    assert _call(top_p=top_p) == DMI_ERR_INVALID
    msg = _msg()
    assert msg.startswith("sample_tokens_guided") and "top_p" in msg, msg


def test_other_argument_errors_are_refused_with_a_message():
    assert _call(nv=8193) == DMI_ERR_INVALID and "8192" in _msg()
    assert _call(z=None) == DMI_ERR_INVALID and "null" in _msg()
    assert _call(next_tok=None) == DMI_ERR_INVALID and "null" in _msg()
    assert _call(Bc=0) == DMI_ERR_INVALID and "Bc" in _msg()
    assert _call(Bc=-3) == DMI_ERR_INVALID and "Bc" in _msg()
    assert _call(advance=1) == DMI_ERR_INVALID and "advance needs pos_dev" in _msg()
    assert _msg().startswith("sample_tokens_guided")


# ---------------------------------------------------------------- the restated guided logits
def test_restated_g_rounds_difference_product_and_sum_separately():
    zc = np.array([1.0, 0.1, -3.0, 2.5], np.float32)
    zu = np.array([0.5, 0.3, -3.0, -1.25], np.float32)
    assert guided_logits(zc, zu, 1.0).tolist() == zc.tolist()
    g = guided_logits(zc, zu, 3.0)
    assert g.dtype == np.float32
    d = (zc - zu).astype(np.float32)
    assert g.tolist() == (zc + (np.float32(2) * d).astype(np.float32)).astype(np.float32).tolist()
    assert g[2] == zc[2]                                         # equal rows: guidance changes nothing
    # scale 0 draws from the unconditional row (up to the rounding of d)
    assert np.allclose(guided_logits(zc, zu, 0.0), zu, atol=1e-6)


def test_guidance_sharpens_the_kept_set_towards_the_caption():
    zc = np.array([2.0, 1.0, 0.0, 0.0], np.float32)
    zu = np.array([0.0, 1.0, 2.0, 0.0], np.float32)
    assert guided_keep(zc, zu, 1.0, 1.0, 0, 0.6).tolist() == [True, False, False, False]
    assert guided_keep(zc, zu, 0.0, 1.0, 0, 0.6).tolist() == [False, False, True, False]
    assert guided_keep(zc, zu, 3.0, 1.0, 2, 1.0).tolist() == [True, True, False, False]     # g = [6, 1, -4, 0]


# ---------------------------------------------------------------- generate_dalle.py argument checks (no GPU)
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "generate_dalle.py")] + list(args), cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=120)


def test_generate_cli_help_names_the_flag():
    r = _cli("--help")
    assert r.returncode == 0 and "--guidance-scale" in r.stdout, r.stderr


@pytest.mark.parametrize("args, msg", [
    (["--from-eval", "2", "--guidance-scale", "-1"], "--guidance-scale must be finite and >= 0"),
    (["--from-eval", "2", "--guidance-scale", "nan"], "--guidance-scale must be finite and >= 0"),
    (["--from-eval", "2", "--guidance-scale", "inf"], "--guidance-scale must be finite and >= 0"),
    (["--from-eval", "2", "--guidance-scale", "2", "--batch", "3"], "batch must be even"),
])
def test_generate_cli_rejects_bad_guidance_arguments_before_the_gpu(args, msg):
    r = _cli("--model", "dalle_example", *args)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert msg in r.stderr, r.stderr[-2000:]
    assert "Traceback" not in r.stderr


# ---------------------------------------------------------------- caption dropout
T, TV = 12, 60


def _params(**kw):
    p = dict(dataset=dict(train_path="synthetic", eval_path="synthetic", image_size=8), n_channels=3, text_seq_len=T,
             text_vocab_size=TV, padding_id=TV - 3, train_batch_size=16, eval_batch_size=16)
    p.update(kw)
    return p


def _take(params, n, eval=False):
    from src.input_fns import dalle_input_fn
    it = dalle_input_fn(params, eval=eval)
    out = [next(it) for _ in range(n)]
    return np.concatenate([o[0].numpy() for o in out]), np.concatenate([o[1].numpy() for o in out])


def test_caption_dropout_absent_or_zero_is_bit_identical():
    img0, cap0 = _take(_params(), 4)
    for p in (0, 0.0):
        img, cap = _take(_params(caption_dropout=p), 4)
        assert np.array_equal(img, img0) and np.array_equal(cap, cap0) and cap.dtype == cap0.dtype


def test_caption_dropout_replaces_whole_captions_and_nothing_else():
    pad = TV - 3
    img0, cap0 = _take(_params(), 6)
    img, cap = _take(_params(caption_dropout=0.4), 6)
    assert np.array_equal(img, img0) and cap.dtype == cap0.dtype and cap.shape == cap0.shape
    dropped = (cap != cap0).any(1)
    assert 0 < dropped.sum() < len(cap)
    assert (cap[dropped] == pad).all()                            # a dropped row is the null caption
    assert np.array_equal(cap[~dropped], cap0[~dropped])          # every other caption is the one the stream read
    # reproducible, and the padding rule of the pipeline when padding_id is unset
    assert np.array_equal(_take(_params(caption_dropout=0.4), 6)[1], cap)
    _, capn = _take(_params(caption_dropout=0.4, padding_id=None), 6)
    _, capn0 = _take(_params(padding_id=None), 6)
    dn = (capn != capn0).any(1)
    assert dn.any() and (capn[dn] == TV - 1).all()


def test_caption_dropout_leaves_eval_untouched():
    img0, cap0 = _take(_params(), 4, eval=True)
    img, cap = _take(_params(caption_dropout=0.9), 4, eval=True)
    assert np.array_equal(img, img0) and np.array_equal(cap, cap0)


def test_caption_dropout_fraction_is_binomial():
    p, pad = 0.25, TV - 3
    n_batches = 250                                               # 4000 captions
    _, cap0 = _take(_params(), n_batches)
    _, cap = _take(_params(caption_dropout=p), n_batches)
    n = len(cap)
    assert n == 4000
    # a synthetic caption of length T with no padding cannot show a drop only if it is already all padding: never (ids < pad)
    dropped = (cap == pad).all(1) & ~(cap0 == pad).all(1)
    sigma = math.sqrt(p * (1 - p) / n)
    assert abs(dropped.mean() - p) <= 5 * sigma, (dropped.mean(), sigma)


@pytest.mark.parametrize("p", [-0.1, 1.0, 1.5, float("nan"), "0.1", True])
def test_caption_dropout_outside_the_unit_interval_is_refused(p):
    from src.input_fns import dalle_input_fn
    with pytest.raises(ValueError, match="caption_dropout"):
        dalle_input_fn(_params(caption_dropout=p))
    with pytest.raises(ValueError, match="caption_dropout"):
        dalle_input_fn(_params(caption_dropout=p), eval=True)


def test_sampler_argument_check_refuses_bad_guidance_arguments_without_a_device():
    """check_sample_args, the argument check of DalleEngine.sample_image_tokens: the cases of
    test_guidance_engine_gpu.py::test_guidance_refusals, same exception types and key words"""
    import torch
    from src.dalle_mtf.engine import check_sample_args
    T, P, TV, IV, B = 16, 48, 60, 64, 4
    BC = B // 2
    text, cap = torch.zeros(B, T, dtype=torch.int32), torch.zeros(BC, T, dtype=torch.int32)

    def check(text, B=B, **kw):
        return check_sample_args(B, T, P, TV, IV, text, **kw)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="guidance_scale"):
            check(cap, guidance_scale=bad)
    with pytest.raises(ValueError, match="text must be"):
        check(text, guidance_scale=2.0)                      # B rows of text where B / 2 are wanted
    for bad in (torch.zeros(T + 1, dtype=torch.int32), torch.zeros(B, T, dtype=torch.int32), torch.zeros(BC, T, 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match="uncond_text must be"):
            check(cap, guidance_scale=2.0, uncond_text=bad)
    with pytest.raises(ValueError, match="integer"):
        check(cap, uncond_text=torch.zeros(T))
    for bad in (TV, -1):
        with pytest.raises(ValueError, match="uncond_text ids"):
            check(cap, uncond_text=torch.full((T,), bad, dtype=torch.int32))
    with pytest.raises(ValueError, match="image_prefix"):
        check(cap, guidance_scale=2.0, image_prefix=torch.zeros(B, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="even"):
        check(text[:1], B=3, guidance_scale=2.0)
    # what it hands on: B / 2 rows, the null caption from padding_id (text_vocab_size - 1 without one), the arguments as given
    a = check(cap, guidance_scale=2.0, top_p=0.5, image_prefix=torch.zeros(BC, 3, dtype=torch.int64))
    assert (a.rows, a.guided, a.guidance_scale, a.top_p, a.prefix_len) == (BC, True, 2.0, 0.5, 3)
    assert a.uncond_text.dtype == torch.int32 and a.uncond_text.tolist() == [TV - 1] * T
    assert check(cap, guidance_scale=2.0, padding_id=TV - 2).uncond_text.tolist() == [TV - 2] * T
    a = check(text)
    assert (a.rows, a.guided, a.guidance_scale, a.top_p, a.uncond_text, a.image_prefix, a.prefix_len) == (B, False, 1.0, 1.0, None, None, 0)
