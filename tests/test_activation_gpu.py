"""GELU feed-forward on the GPU (DALLE activation_fn="gelu", DESIGN.md §4 "GELU"): the two GELU epilogues of the NT products on
every tile kernel the dispatch can pick for them, the decode path's LayerNorm + dense, the engine against the GELU oracle, the
batch additivity of its gradient at the benchmark batch, its samplers, checkpoints and the command-line workflow; and ReLU runs
unchanged by the new option."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dalle_hip as dh  # noqa: E402  (path set up by conftest)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gelu_ref import gelu, gelu_grad  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = 2.0 ** -24
# options that force one tile kernel of launch_nt (the full-row kernel gemm_ntr is built without the GELU epilogues: ntr = 0 keeps the
# BIAS reference on the same kernel as the GELU product for N = 512 shapes too)
PATHS = {
    "skinny": dict(skinny=1, ntr=0),
    "nt2": dict(skinny=0, ntr=0, nt8p=0, nt8=0, nt4=0),
    "nt4": dict(skinny=0, ntr=0, nt8p=0, nt8=0, nt4=2),
    "nt8": dict(skinny=0, ntr=0, nt8p=0, nt8=2),
    "nt8p": dict(skinny=0, ntr=0, nt8p=2),
}


class _options:
    def __init__(self, opts):
        self.opts = opts

    def __enter__(self):
        self.saved = {k: dh.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            dh.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            dh.set_option(k, v)


def _ulp_bf16(x):
    """the bf16 unit in the last place at |x| (float64 tensor): 2^(e - 7), e = floor(log2 |x|); the smallest normal's below it"""
    ax = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(ax)) - 7)


def _operands(M, N, K, seed):
    """|a| = |A . B^T + bias| up to ~30: the saturation of sigmoid(2u) on both sides and everything in between"""
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    Bt = (torch.randn(N, K, generator=g) * (8.0 / K ** 0.5)).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(N, generator=g) * 2).to(torch.bfloat16).to(DEV)
    dY = (torch.randn(M, K, generator=g)).to(torch.bfloat16).to(DEV)
    return A, Bt, bias, dY


def _fp32_product(A, Bt):
    """fp32 A . Bt^T and the bound of its summation-order error against any other fp32 order: 2 K eps32 (|A| . |Bt|^T)"""
    a, b = A.double(), Bt.double()
    return a @ b.t(), 2 * A.shape[1] * EPS32 * (a.abs() @ b.abs().t())


@pytest.mark.parametrize("path,M,N,K", [
    ("skinny", 7, 1024, 512), ("skinny", 32, 2048, 256),
    ("nt2", 333, 1000, 256), ("nt4", 333, 1000, 256), ("nt8", 333, 1000, 256), ("nt8p", 333, 1000, 256),
    ("nt2", 300, 512, 128), ("nt8p", 600, 512, 128),
    ("nt8p", 40960, 2048, 512),      # FFN-1 / FFN-2 input gradient at dalle_example B = 32: the production kernel
])
def test_gelu_epilogues_vs_fp32_math(path, M, N, K):
    A, Bt, bias, dY = _operands(M, N, K, seed=M + N + K)
    C = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    pre = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    ref_pre = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    dH = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    with _options(PATHS[path]):
        dh.gemm_nt_gelu(A, K, Bt, K, C, N, M, N, K, bias, pre, N)
        dh.gemm_nt(A, K, Bt, K, ref_pre, N, M, N, K, dh.GEMM_BIAS, bias=bias)
        # the input gradient of FFN-2: dY [M, K] . W2 [N, K]^T, times gelu'(pre)
        dh.gemm_nt_gelu_grad(dY, K, Bt, K, dH, N, M, N, K, pre, N)
    torch.cuda.synchronize()
    # pre: what the same kernel stores under GEMM_BIAS, bit for bit
    assert torch.equal(pre.view(torch.int16), ref_pre.view(torch.int16)), path
    # C = bf16(gelu(a)), a the kernel's fp32 acc + bias: within 1 bf16 ulp of gelu(a') for the fp32 a' computed here, plus what
    # the two summation orders can differ by (|gelu'| <= 1.13)
    acc, err = _fp32_product(A, Bt)
    a = acc + bias.double()
    ref = gelu(a)
    tol = _ulp_bf16(ref) + 1.13 * err + 1e-30
    bad = (C.double() - ref).abs() > tol
    assert not bad.any(), f"{path} gelu: {int(bad.sum())} of {bad.numel()} outside 1 ulp; worst {float(((C.double() - ref).abs() / tol).max()):.3g} x tol"
    # saturation on both sides was exercised, and reproduced exactly
    assert float(a.min()) < -15 and float(a.max()) > 15, (float(a.min()), float(a.max()))
    big = a > 12       # sigmoid(2u) = 1 exactly in fp32: C = bf16(a) = pre
    assert torch.equal(C[big].view(torch.int16), pre[big].view(torch.int16))
    assert (C[a < -12].double().abs() < 1e-20).all()
    # dH = bf16(dY . W2^T * gelu'(pre)), gelu' in fp32 of the bf16 pre (~1e-6 absolute from exp2 / rcp)
    acc2, err2 = _fp32_product(dY, Bt)
    gp = gelu_grad(pre.double())
    ref2 = acc2 * gp
    tol2 = _ulp_bf16(ref2) + gp.abs() * err2 + 4e-6 * acc2.abs() + 1e-30
    bad2 = (dH.double() - ref2).abs() > tol2
    assert not bad2.any(), f"{path} gelu grad: {int(bad2.sum())} of {bad2.numel()} outside; worst {float(((dH.double() - ref2).abs() / tol2).max()):.3g} x tol"


def test_gelu_entry_points_refuse_bad_pre():
    M, N, K = 64, 256, 128
    A, Bt, bias, _ = _operands(M, N, K, seed=3)
    C = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    pre = torch.empty(M * N + 8, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(dh.DalleHipError, match="ldpre"):
        dh.gemm_nt_gelu(A, K, Bt, K, C, N, M, N, K, bias, pre, N - 8)
    with pytest.raises(dh.DalleHipError, match="aligned"):
        dh.gemm_nt_gelu_grad(A, K, Bt, K, C, N, M, N, K, pre.data_ptr() + 2, N)
    with pytest.raises(dh.DalleHipError, match="null pre"):
        dh.gemm_nt_gelu_grad(A, K, Bt, K, C, N, M, N, K, None, N)


@pytest.mark.parametrize("M,N,K", [(1, 1024, 256), (32, 2048, 512)])
def test_ln_gemm_nt_gelu_vs_layernorm_dense_gelu(M, N, K):
    """the decode path's LayerNorm + dense + GELU: the same kernel with BIAS alone gives the pre-activation (rounded to bf16)"""
    g = torch.Generator().manual_seed(M + N)
    X = (torch.randn(M, K, generator=g) * 3 + 1).to(torch.bfloat16).to(DEV)
    gamma = (1 + 0.2 * torch.randn(K, generator=g)).to(torch.bfloat16).to(DEV)
    beta = (0.1 * torch.randn(K, generator=g)).to(torch.bfloat16).to(DEV)
    W = (torch.randn(N, K, generator=g) * (8.0 / K ** 0.5)).to(torch.bfloat16).to(DEV)
    bias = (torch.randn(N, generator=g) * 2).to(torch.bfloat16).to(DEV)
    C = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    P = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
    dh.ln_gemm_nt(X, K, gamma, beta, W, K, C, N, M, N, K, dh.GEMM_BIAS | dh.GEMM_GELU, bias=bias)
    dh.ln_gemm_nt(X, K, gamma, beta, W, K, P, N, M, N, K, dh.GEMM_BIAS, bias=bias)
    torch.cuda.synchronize()
    # P = bf16(a): |a - P| <= ulp(P) / 2, so |gelu(a) - gelu(P)| <= 1.13 ulp(P) / 2; C adds its own rounding (<= 1 ulp here)
    ref = gelu(P.double())
    tol = _ulp_bf16(ref) + 0.57 * _ulp_bf16(P.double()) + 1e-30
    assert ((C.double() - ref).abs() <= tol).all()
    # and against LayerNorm + dense in fp32 math (bf16 LN output, as the kernel rounds it)
    xf = X.double()
    xn = ((xf - xf.mean(1, keepdim=True)) / torch.sqrt(xf.var(1, unbiased=False, keepdim=True) + 1e-5) * gamma.double() + beta.double())
    a = xn.to(torch.bfloat16).double() @ W.double().t() + bias.double()
    rel = float((C.double() - gelu(a)).norm() / gelu(a).norm())
    assert rel < 1e-2, rel


# ------------------------------------------------------------------ the engine
@pytest.mark.parametrize("n_embd,n_heads,P,recompute", [(256, 2, 112, False), (256, 2, 112, True), (128, 2, 256, False), (256, 4, 256, True)])
def test_engine_gelu_step_vs_gelu_oracle(n_embd, n_heads, P, recompute):
    """the compare_step pattern against the fp32 step oracle with activation="gelu"; the bounds of the ReLU tests of the same shapes
    (check_report's defaults: tests/parity.py smoke_step at head dim 128, test_engine_step_head_dim64_vs_oracle at 64)"""
    from engine_case import HP
    from parity import check_report, compare_step
    hp = dict(HP, activation_fn="gelu", recompute_grad=recompute)
    rep = compare_step(n_embd=n_embd, n_heads=n_heads, T=16, P=P, hp=hp, ref_kw=dict(activation="gelu"))
    check_report(rep)


def test_gelu_oracle_differs_from_relu_oracle():
    """the switch is in effect: the GELU oracle's loss is not the ReLU oracle's (so the parity test above pins the activation)"""
    import dalle_step_ref as sref
    from oracle import dalle_oracle as do
    cfg = do.DalleConfig(128, 60, 64, 16, 112, 1, 1)
    P0 = do.init_params(cfg, seed=3, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(2, 16, 60, seed=1), do.synthetic_image_tokens(2, 112, 64, seed=2), 60)
    lr, _ = do.loss_and_grads(P0, tokens, cfg)
    lg, _ = sref.loss_and_grads(P0, tokens, cfg, activation="gelu")
    assert abs(lr - lg) > 1e-4 * abs(lr), (lr, lg)


def _headline_engine(B, act):
    from src.dalle_mtf.engine import DalleEngine
    eng = DalleEngine(512, 6, 4, 50258, 512, 256, 1024, batch_size=B, global_batch_size=32,
                      hparams=dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0, activation_fn=act))
    eng.init_params(seed=1234)
    eng.global_step = 1500
    return eng


def test_gelu_benchmark_batch_gradient_equals_the_sum_of_the_two_sequence_gradients():
    """dalle_example at B = 32 runs FFN-1 / the FFN-2 input gradient on the persistent 256x256 kernel's GELU epilogues: its
    gradient is the sum of the sixteen B = 2 gradients (the bounds of test_headline_parity_gpu.py's ReLU test)"""
    from oracle import dalle_oracle as do
    B = 32
    tokens = torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, 256, 50258, seed=1),
                                                 do.synthetic_image_tokens(B, 1024, 512, seed=2), 50258)).cuda()
    big = _headline_engine(B, "gelu")
    assert big.hpre is not None and not big.use_relu_bits
    big.forward(tokens, need_grad=True)
    big.backward(allreduce=False)
    torch.cuda.synchronize()
    gb = big.export_reference(big.g)
    del big
    torch.cuda.empty_cache()
    small = _headline_engine(2, "gelu")
    acc = None
    for i in range(0, B, 2):
        small.forward(tokens[i:i + 2].contiguous(), need_grad=True)
        small.backward(allreduce=False)
        torch.cuda.synchronize()
        gs = small.export_reference(small.g)
        acc = {k: v.astype(np.float64) for k, v in gs.items()} if acc is None else {k: acc[k] + gs[k] for k in acc}
    del small
    torch.cuda.empty_cache()
    worst = max((float(np.linalg.norm(gb[k] - acc[k]) / (np.linalg.norm(acc[k]) + 1e-30)), k) for k in gb)
    head = {k: float(np.linalg.norm(gb[k] - acc[k]) / (np.linalg.norm(acc[k]) + 1e-30)) for k in gb if "to_logits" in k}
    print("GELU: B = 32 gradient vs the sum of sixteen B = 2 gradients: worst", worst, "head", head, flush=True)
    assert worst[0] <= 5e-3, worst
    assert all(v <= 1e-3 for v in head.values()), head


def _small(act, seed=9, **hp):
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    T, P, tv, iv, B = 16, 112, 60, 64, 2
    cfg = do.DalleConfig(512, tv, iv, T, P, 2, 4)
    eng = DalleEngine(512, 2, 4, tv, iv, T, P, batch_size=B,
                      hparams=dict(dict(lr=1e-3, train_steps=10, warmup_steps=1, gradient_clipping=1.0), **hp, **({"activation_fn": act} if act else {})))
    eng.load_reference_params(do.init_params(cfg, seed=seed, perturb=0.05))
    toks = torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, T, tv, seed=1),
                                               do.synthetic_image_tokens(B, P, iv, seed=2), tv)).cuda()
    return eng, toks


def test_gelu_samplers_agree():
    """greedy tokens under GELU: graph-replayed decode + draw, host-launched draw, ungraphed decode (all on the BIAS | GELU decode
    products) and the one-forward-per-token sampler (the training kernels' GELU epilogue) -- as test_head_dim64_samplers_agree"""
    eng, toks = _small("gelu")
    text = toks[:, :16].contiguous()
    a = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True)
    a2 = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True, fused_sampling=False)
    a3 = eng.sample_image_tokens(text, temperature=0.0, kv_cache=True, decode_graph=False)
    assert torch.equal(a, a2) and torch.equal(a, a3)
    b = eng.sample_image_tokens(text, temperature=0.0, kv_cache=False)
    agree = float((a == b).float().mean())
    print("GELU: cached vs uncached greedy tokens agree on", agree, flush=True)
    assert int((a != b).any(1).sum()) == 0 or agree >= 0.5, agree
    # and the GELU model is not the ReLU one: its greedy samples differ
    relu, _ = _small(None)
    c = relu.sample_image_tokens(text, temperature=0.0, kv_cache=True)
    assert not torch.equal(a, c)


def test_relu_option_is_bit_identical_to_the_default():
    runs = []
    for act in (None, "relu"):
        eng, toks = _small(act)
        assert eng.activation == "relu" and eng.hpre is None
        for _ in range(2):
            eng.train_step(toks)
        torch.cuda.synchronize()
        runs.append(eng.p.detach().cpu().clone())
        del eng
    assert torch.equal(runs[0], runs[1])


def test_gelu_checkpoint_resumes_bit_identically_and_relu_refuses_it(tmp_path):
    full, toks = _small("gelu")
    for _ in range(3):
        full.train_step(toks)
    first, _ = _small("gelu")
    for _ in range(2):
        first.train_step(toks)
    path = str(tmp_path / "ck.pt")
    torch.save({"dalle": first.state_dict()}, path)
    sd = torch.load(path)["dalle"]
    assert sd["activation_fn"] == "gelu"
    resumed, _ = _small("gelu", seed=1)
    resumed.load_state_dict(sd)
    resumed.train_step(toks)
    torch.cuda.synchronize()
    assert torch.equal(full.p.cpu(), resumed.p.cpu())
    relu, _ = _small("relu")
    with pytest.raises(ValueError, match="gelu"):
        relu.load_state_dict(sd)
    old = {k: v for k, v in relu.state_dict().items() if k != "activation_fn"}   # a checkpoint from before the key: ReLU
    relu.load_state_dict(old)
    with pytest.raises(ValueError, match="relu"):
        resumed.load_state_dict(old)


# ------------------------------------------------------------------ the command line
def _shards(tmp_path, n=8, size=32):
    import io
    from PIL import Image
    sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
    from src.data.create_tfrecords import TFRecordWriter, serialize_example
    rng = np.random.default_rng(0)
    w = TFRecordWriter(str(tmp_path / "pairs_0.tfrecords"))
    for _ in range(n):
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, size=(size, size, 3), dtype=np.uint8)).save(buf, format="JPEG", quality=90)
        w.write(serialize_example(buf.getvalue(), rng.integers(0, 50257, size=int(rng.integers(1, 300))).tolist()))
    w.close()
    return str(tmp_path / "pairs_*.tfrecords")


def _run(args, cwd):
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable] + args, cwd=cwd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def test_gelu_config_trains_resumes_and_samples_from_the_cli(tmp_path):
    glob = _shards(tmp_path)
    ds = {"train_path": glob, "eval_path": glob, "image_size": 32, "tfrecords": True}
    vae = json.load(open(os.path.join(ROOT, "configs", "vae_example.json")))
    vae.update(dataset=ds, model_path=str(tmp_path / "no_vae_run"))
    json.dump(vae, open(tmp_path / "vae.json", "w"))
    cfg = json.load(open(os.path.join(ROOT, "configs", "dalle_example.json")))
    cfg.update(dataset=ds, vae_model=str(tmp_path / "vae.json"), allow_random_vae=True, train_batch_size=4, eval_batch_size=4,
               predict_batch_size=4, train_steps=2, steps_per_checkpoint=2, eval_steps=1, model_path=str(tmp_path / "run"),
               iterations=1, n_layers=1, n_embd=256, n_heads=2, warmup_steps=1, activation_fn="gelu")
    path = str(tmp_path / "gelu.json")
    json.dump(cfg, open(path, "w"))
    out = _run([os.path.join(ROOT, "train_dalle.py"), "--model", path], str(tmp_path))
    assert "step 2" in out, out[-1500:]
    cks = [f for f in os.listdir(tmp_path / "run") if f.endswith(".pt")]
    assert cks, os.listdir(tmp_path / "run")
    sd = torch.load(os.path.join(tmp_path / "run", sorted(cks)[-1]), map_location="cpu", weights_only=False)
    assert sd["dalle"]["activation_fn"] == "gelu", list(sd)
    cfg["train_steps"] = 3
    json.dump(cfg, open(path, "w"))
    out = _run([os.path.join(ROOT, "train_dalle.py"), "--model", path], str(tmp_path))      # resumes from step 2
    assert "Current step: 2" in out, out[-1500:]
    _run([os.path.join(ROOT, "generate_dalle.py"), "--model", path, "--from-eval", "2", "--samples-per-caption", "1",
          "--batch", "4", "--top-p", "0.9", "--out", str(tmp_path / "gen")], str(tmp_path))
    toks = np.load(tmp_path / "gen" / "tokens.npy")
    assert toks.shape == (2, 16) and toks.min() >= 0 and toks.max() < 512
    # a ReLU config refuses the GELU run's checkpoint
    cfg.update(activation_fn="relu", train_steps=4)
    json.dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_dalle.py"), "--model", path], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode != 0 and "gelu" in (r.stdout + r.stderr)
