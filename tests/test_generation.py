"""Generation, CPU side: the nucleus-draw C ABI (declared, exported, bound; argument errors come back as a status and a message
before anything is launched -- the pointers below are never dereferenced), its compile-time resources, the numpy restatement
of the nucleus set on hand-built rows, and generate_dalle.py's argument checks (all before any GPU is touched)."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dalle_hip as dh  # noqa: E402
from nucleus_ref import nucleus_keep, quantised_q  # noqa: E402

FAKE = ctypes.c_void_p(0x10000)
DMI_ERR_INVALID = -1


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def _call(z=FAKE, nv=64, top_p=0.9, advance=0, pos_dev=None, next_tok=FAKE):
    return dh.lib().dmi_sample_tokens_p(z, nv, None, 2, nv, 1.0, 0, 0, top_p, None, 0, pos_dev, advance, 0, next_tok, None, 0, 0,
                                        None, None)


def test_nucleus_entry_point_is_declared_exported_and_bound():
    L = dh.lib()
    assert "dmi_sample_tokens_p" in dh.declared_symbols()
    fn = L.dmi_sample_tokens_p
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 20
    assert len(L.dmi_sample_tokens.argtypes) == 18          # the top-k draw keeps its signature
    assert callable(dh.sample_tokens_p)
    prm = dh.sample_params(0.5, 7, (3 << 32) | 9, top_p=0.25)
    assert prm.shape == (6,) and prm.numpy().view(np.uint32).tolist() == [
        int(np.array([2.0], np.float32).view(np.uint32)[0]), 7, 9, 3, int(np.array([0.25], np.float32).view(np.uint32)[0]), 0]


@pytest.mark.parametrize("top_p", [0.0, -0.1, 1.5, float("nan"), float("inf")])
def test_top_p_outside_the_unit_interval_is_refused(top_p):
    assert _call(top_p=top_p) == DMI_ERR_INVALID
    msg = _msg()
    assert msg.startswith("sample_tokens_p") and "top_p" in msg, msg
    with pytest.raises(dh.DalleHipError):
        dh._check(_call(top_p=top_p), "sample_tokens_p")


def test_other_argument_errors_are_refused_with_a_message():
    assert _call(nv=8193) == DMI_ERR_INVALID and "8192" in _msg()
    assert _call(z=None) == DMI_ERR_INVALID and "null" in _msg()
    assert _call(next_tok=None) == DMI_ERR_INVALID and "null" in _msg()
    assert _call(advance=1) == DMI_ERR_INVALID and "advance needs pos_dev" in _msg()


def test_nucleus_kernel_uses_no_scratch_and_no_spills():
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
                                     lds=g(r"LDS Size \[bytes/block\]"), occupancy=g(r"Occupancy \[waves/SIMD\]"))
    (k,) = [k for k in usage if "sample_tokens_p_kernel" in k]
    u = usage[k]
    assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, u
    # two 32 KB tables: two 256-thread blocks fit a CU's 160 KB, so a B <= 128 launch is resident at once on 256 CUs
    assert u["lds"] <= 80 * 1024 and u["occupancy"] >= 2, u
    # the plain instance of the same body: one 32 KB key table and the small reduce arrays, not the nucleus form's second table
    (k,) = [k for k in usage if "sample_tokens_kernel" in k]
    u = usage[k]
    assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, u
    assert u["lds"] <= 40 * 1024, u


@pytest.mark.parametrize("temperature", [0.0, 0.5, 1.0])
def test_engine_parameter_words_of_the_plain_draw(temperature):
    """the engine fills the plain draw's device parameter block through dh.sample_params: the four words it used to pack by hand"""
    from src.dalle_mtf.engine import Draw, draw_params
    top_k, seed = 7, (5 << 32) | 0x9abcdef1
    inv_t = np.array([1.0 / temperature if temperature > 0 else 0.0], dtype=np.float32).view(np.uint32)[0]
    want = np.array([inv_t, int(top_k), seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint32).view(np.int32)
    got = draw_params(Draw(nucleus=False, guided=False, logp=False), temperature, top_k, seed, top_p=1.0, guidance_scale=1.0)
    assert got.dtype == dh.sample_params(temperature, top_k, seed).dtype and got.shape == (4,)
    assert got.tolist() == want.tolist() == dh.sample_params(temperature, top_k, seed).tolist()
    # the other variants carry six words: top_p, and the scale only under guidance
    assert draw_params(Draw(True, False, True), temperature, top_k, seed, 0.9, 2.0).tolist() == \
        dh.sample_params(temperature, top_k, seed, 0.9).tolist()
    assert draw_params(Draw(True, True, False), temperature, top_k, seed, 0.9, 2.0).tolist() == \
        dh.sample_params(temperature, top_k, seed, 0.9, guidance_scale=2.0).tolist()


# ---------------------------------------------------------------- the restated nucleus set on hand-built rows
def _q(v):
    e = np.exp(np.asarray(v, np.float64) - max(v))
    return e / e.sum()


def test_nucleus_top_p_one_is_the_top_k_set():
    v = np.array([3.0, 1.0, 2.0, 2.0, -1.0, 0.5], np.float32)
    assert nucleus_keep(v, 0, 1.0).all()
    assert nucleus_keep(v, 3, 1.0).tolist() == [True, False, True, True, False, False]
    assert nucleus_keep(v, 2, 1.0).tolist() == [True, False, True, True, False, False]    # ties of the k-th value kept


def test_nucleus_tiny_top_p_keeps_the_maximum_alone():
    v = np.array([0.0, 4.0, 1.0, 3.9, -2.0], np.float32)
    assert nucleus_keep(v, 0, 1e-6).tolist() == [False, True, False, False, False]


def test_nucleus_ties_at_tau_are_all_kept():
    # q = 0.4, 0.2, 0.2, 0.2 (as logits): the shortest prefix reaching 0.5 ends inside the tie; all three tied entries stay
    v = np.log(np.array([0.4, 0.2, 0.2, 0.2], np.float64)).astype(np.float32)
    assert nucleus_keep(v, 0, 0.5).tolist() == [True, True, True, True]
    assert nucleus_keep(v, 0, 0.39).tolist() == [True, False, False, False]
    v = np.array([2.0, 1.0, 1.0, 0.0, -5.0], np.float32)
    q = _q(v)
    assert q[0] < 0.6 < q[0] + q[1] < q[0] + q[1] + q[2] < 0.99
    assert nucleus_keep(v, 0, 0.6).tolist() == [True, True, True, False, False]      # the prefix ends at entry 1; its tie 2 stays


def test_nucleus_is_the_shortest_prefix_reaching_top_p():
    rng = np.random.default_rng(0)
    for _ in range(200):
        nv = int(rng.integers(2, 300))
        v = (rng.standard_normal(nv) * 3).astype(np.float32)
        p = float(rng.uniform(0.05, 0.99))
        keep = nucleus_keep(v, 0, p)
        u = quantised_q(v, np.ones(nv, bool)).astype(np.float64)
        order = np.argsort(-v, kind="stable")
        mass = np.cumsum(u[order]) / u.sum()
        n = int(np.argmax(mass >= np.float32(p) * (1 - 1e-12)))    # shortest prefix (distinct values: no ties)
        assert keep.sum() == n + 1 and keep[order[:n + 1]].all(), (nv, p)
        assert abs(_q(v)[keep].sum() - mass[n]) < 1e-6


def test_nucleus_after_top_k():
    v = np.array([5.0, 4.9, 4.8, 0.0, 0.0, -1.0], np.float32)
    # top-k = 2 leaves {0, 1}; renormalised over them the maximum has ~0.52 of the mass
    assert nucleus_keep(v, 2, 0.5).tolist() == [True, False, False, False, False, False]
    assert nucleus_keep(v, 2, 0.6).tolist() == [True, True, False, False, False, False]
    assert nucleus_keep(v, 0, 0.6).tolist() == [True, True, False, False, False, False]
    assert nucleus_keep(v, 0, 0.7).tolist() == [True, True, True, False, False, False]


def test_fixed_point_mass_is_order_free():
    rng = np.random.default_rng(1)
    v = (rng.standard_normal(4096) * 2).astype(np.float32)
    u = quantised_q(v, np.ones(4096, bool))
    assert int(u.max()) == 2 ** 31 and int(u.sum()) == int(u[rng.permutation(4096)].sum())
    target = math.ceil(float(np.float32(0.9)) * float(int(u.sum())))
    assert 0 < target <= int(u.sum())


# ---------------------------------------------------------------- generate_dalle.py argument checks (no GPU)
def _cli(*args):
    env = dict(os.environ, PYTHONPATH=ROOT, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "generate_dalle.py")] + list(args), cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=120)


def test_generate_cli_help():
    r = _cli("--help")
    assert r.returncode == 0, r.stderr
    for flag in ("--model", "--caption-ids", "--captions", "--from-eval", "--image-prefix", "--samples-per-caption", "--top-p",
                 "--top-k", "--temperature", "--seed", "--out", "--batch", "--checkpoint"):
        assert flag in r.stdout, flag


@pytest.mark.parametrize("args, msg", [
    (["--from-eval", "2", "--image-prefix", "16"], "--image-prefix must lie in [0, image_seq_len = 16)"),
    (["--from-eval", "2", "--image-prefix", "-1"], "--image-prefix"),
    (["--from-eval", "2", "--captions", "x.txt"], "not allowed with"),
    (["--from-eval", "2", "--top-p", "0"], "--top-p must lie in (0, 1]"),
    (["--from-eval", "2", "--top-p", "1.5"], "--top-p must lie in (0, 1]"),
    (["--from-eval", "2", "--top-p", "nan"], "--top-p must lie in (0, 1]"),
    (["--from-eval", "2", "--samples-per-caption", "0"], "--samples-per-caption"),
    (["--from-eval", "2", "--top-k", "-3"], "--top-k"),
    (["--caption-ids", "/nonexistent/ids.npy"], "not found"),
    (["--caption-ids", "/nonexistent/ids.npy", "--image-prefix", "3"], "--image-prefix needs --from-eval"),
    ([], "one of the arguments"),
])
def test_generate_cli_rejects_bad_arguments_before_the_gpu(args, msg):
    r = _cli("--model", "dalle_example", *args)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert msg in r.stderr, r.stderr[-2000:]
    assert "Traceback" not in r.stderr


def test_generate_cli_rejects_a_caption_file_without_a_gpt2_vocabulary(tmp_path):
    from src.data import get_tokenizer
    from src.data.tokenizer_utils import _OfflineTokenizer
    if not isinstance(get_tokenizer(None, vocab_size=50258), _OfflineTokenizer):
        pytest.skip("a local GPT-2 vocabulary is installed: captions can be tokenised")
    f = tmp_path / "c.txt"
    f.write_text("a red bird\n")
    r = _cli("--model", "dalle_example", "--captions", str(f))
    assert r.returncode == 2 and "GPT-2 vocabulary" in r.stderr, r.stderr[-2000:]


def test_generate_cli_rejects_malformed_caption_ids(tmp_path):
    f = tmp_path / "ids.npy"
    np.save(f, np.zeros((3, 17), np.int32))
    r = _cli("--model", "dalle_example", "--caption-ids", str(f))
    assert r.returncode == 2 and "text_seq_len = 256" in r.stderr, r.stderr[-2000:]


def test_sampler_argument_check_refuses_bad_prefixes_and_top_p_without_a_device():
    """check_sample_args, the argument check of DalleEngine.sample_image_tokens: the image_prefix and top_p refusals of
    test_generation_gpu.py (an engine of 3 rows, 48 image positions, 64 image tokens), same exception type and key words"""
    import torch
    from src.dalle_mtf.engine import check_sample_args
    T, P, tv, iv, B = 16, 48, 60, 64, 3
    text = torch.zeros(B, T, dtype=torch.int32)
    for bad in (torch.zeros(3, P, dtype=torch.int32),             # a prefix leaves at least one position to draw
                torch.zeros(2, 4, dtype=torch.int32),             # one row per row of text
                torch.zeros(3, dtype=torch.int32)):
        with pytest.raises(ValueError, match="image_prefix must be"):
            check_sample_args(B, T, P, tv, iv, text, image_prefix=bad)
    for bad in (iv, -1):
        with pytest.raises(ValueError, match="image_prefix ids"):
            check_sample_args(B, T, P, tv, iv, text, image_prefix=torch.full((3, 2), bad, dtype=torch.int32))
    with pytest.raises(ValueError, match="integer"):
        check_sample_args(B, T, P, tv, iv, text, image_prefix=torch.zeros(3, 2))
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            check_sample_args(B, T, P, tv, iv, text, top_p=bad)
    with pytest.raises(AssertionError):
        check_sample_args(B, T, P, tv, iv, text[:2])
    a = check_sample_args(B, T, P, tv, iv, text, image_prefix=[[1, 2], [3, 4], [5, 6]])
    assert a.prefix_len == 2 and a.image_prefix.tolist() == [[1, 2], [3, 4], [5, 6]] and not a.guided and a.rows == B
    assert check_sample_args(B, T, P, tv, iv, text, image_prefix=torch.zeros(3, 0, dtype=torch.int32)).prefix_len == 0
