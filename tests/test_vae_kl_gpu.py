"""KL term and codebook statistics of the discrete VAE on the GPU: dmi_codebook_kl_fwd, dmi_gumbel_softmax_bwd_kl and
dmi_codebook_usage against the float64 specification of tests/vae_kl_ref.py inside its derived bounds (every NC instance and both
sides of each boundary; a lone row, a ragged block of four rows and more rows than one usage slab; five logit families), their
bit-level contracts (two runs equal, weight by value = weight from device memory, weight 0 = dmi_gumbel_softmax_bwd), and the engine:
keys off is today's step launch for launch and bit for bit, loss / gradient with beta > 0, graph = eager under a ramp, the sign of the
effect, and codebook_stats()."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import dalle_hip as dh
import vae_kl_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

T_VALUES = [64, 512, 520, 1024, 1032, 2048, 2056, 4096]      # every NC instance (T <= 512 / 1024 / 2048 / 4096), both sides of each boundary
M_VALUES = [1, 7, 1030]      # a lone row; a ragged last block of four rows; 33 usage slabs of 32 rows, the last with 6
TEMPS = (1.0, 0.5, 0.05)
BETAS = (0.5, 6.6)
SENTINEL = -12345            # as an int16: a bf16 that is never a gradient; as a float: never a row statistic


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _ws(M, T):
    return torch.empty(int(dh.codebook_kl_workspace_bytes(M, T)) + 64, dtype=torch.uint8, device=DEV)


def _kl_fwd(l, extra=3):
    """-> (rowstat [M, 2] on the device, kl as a Python float); `extra` more rows of rowstat must stay untouched"""
    M, T = l.shape
    rs = torch.full((M + extra, 2), float(SENTINEL), dtype=torch.float32, device=DEV)
    kl = torch.full((2,), float(SENTINEL), dtype=torch.float32, device=DEV)
    dh.codebook_kl_fwd(torch.from_numpy(l).to(DEV), rs, kl, M, T, _ws(M, T))
    torch.cuda.synchronize()
    assert (rs[M:] == SENTINEL).all() and kl[1] == SENTINEL, "written past the end"
    return rs[:M].contiguous(), float(kl[0])


@pytest.mark.parametrize("M", M_VALUES)
@pytest.mark.parametrize("T", T_VALUES)
def test_codebook_kl_fwd_vs_float64(T, M):
    for fam in ref.FAMILIES:
        l = ref.family(fam, M, T)
        s = ref.kl_spec(l)
        rs, kl = _kl_fwd(l)
        got = rs.double().cpu().numpy()
        assert np.isfinite(got).all() and np.isfinite(kl), (fam, T, M)
        for name, col, want, bound in (("lse", 0, s["lse"], ref.lse_bound(l)), ("e", 1, s["e"], ref.e_bound(l))):
            err = np.abs(got[:, col] - want)
            print(fam, T, M, name, "worst error / bound:", float(np.max(err / bound)), flush=True)
            assert (err <= bound).all(), (fam, T, M, name, float(err.max()), int(np.argmax(err / bound)))
        print(fam, T, M, "kl error / bound:", abs(kl - s["kl"]) / ref.kl_bound(l), flush=True)
        assert abs(kl - s["kl"]) <= ref.kl_bound(l), (fam, T, M, kl, s["kl"])
        rs2, kl2 = _kl_fwd(l)
        assert torch.equal(rs2.view(torch.int32), rs.view(torch.int32)) and np.float32(kl2).tobytes() == np.float32(kl).tobytes()


def _bwd_kl(dy, p, l, rs, temp, beta, beta_dev=None, temp_dev=None, extra=3):
    M, T = l.shape
    out = torch.full((M + extra, T), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    dh.gumbel_softmax_bwd_kl(dy, p, l, rs, out, M, T, temp, beta, temperature_dev=temp_dev, kl_weight_dev=beta_dev)
    torch.cuda.synchronize()
    assert (_bits(out[M:]) == SENTINEL).all(), "rows >= M written"
    return out[:M]


@pytest.mark.parametrize("M", M_VALUES)
@pytest.mark.parametrize("T", T_VALUES)
def test_gumbel_softmax_bwd_kl_vs_float64(T, M):
    for fam in ref.FAMILIES:
        l = ref.family(fam, M, T)
        dy, p = ref.bwd_inputs(M, T, 0.5, l)
        terms = ref.bwd_terms(dy, p, l)
        rs, _ = _kl_fwd(l)                 # the kernel's own row statistics, as the engine hands them over
        ld, dyd, pd = torch.from_numpy(l).to(DEV), torch.from_numpy(dy).to(DEV).bfloat16(), torch.from_numpy(p).to(DEV).bfloat16()
        for temp in TEMPS:
            plain = torch.empty(M, T, dtype=torch.bfloat16, device=DEV)
            dh.gumbel_softmax_bwd(dyd, pd, plain, M, T, temp)
            zero = _bwd_kl(dyd, pd, ld, rs, temp, 0.0)
            assert torch.equal(_bits(zero), _bits(plain)), (fam, T, M, temp, "kl_weight = 0 is not dmi_gumbel_softmax_bwd")
            for beta in BETAS:
                out = _bwd_kl(dyd, pd, ld, rs, temp, beta)
                want, bound = ref.dlogits_from_terms(terms, temp, beta)
                got = out.double().cpu().numpy()
                assert np.isfinite(got).all(), (fam, T, M, temp, beta)
                err = np.abs(got - want)
                assert (err <= bound).all(), (fam, T, M, temp, beta, float(np.max(err / bound)), np.argwhere(err > bound)[:4].tolist())
                bdev = torch.tensor([beta], dtype=torch.float32, device=DEV)
                tdev = torch.tensor([temp], dtype=torch.float32, device=DEV)
                assert torch.equal(_bits(_bwd_kl(dyd, pd, ld, rs, temp, 0.0, beta_dev=bdev)), _bits(out)), (fam, T, M, temp, beta)
                assert torch.equal(_bits(_bwd_kl(dyd, pd, ld, rs, 1.0, 0.0, beta_dev=bdev, temp_dev=tdev)), _bits(out)), (fam, T, M, temp, beta)
        # the KL gradient alone (dy = 0): its own size decides, not the Gumbel term's bf16 ulp
        z = torch.zeros_like(dyd)
        out = _bwd_kl(z, pd, ld, rs, 1.0, 6.6).double().cpu().numpy()
        want, bound = ref.dlogits_from_terms(dict(terms, G=0.0 * terms["G"], Eg=0.0 * terms["Eg"]), 1.0, 6.6)
        assert (np.abs(out - want) <= bound).all(), (fam, T, M, "dy = 0")


def _run_usage(M, T, l=None, rs=None, idx=None):
    q = torch.full((T + 8,), float(SENTINEL), dtype=torch.float32, device=DEV)
    c = torch.full((T + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    dh.codebook_usage(l, rs, idx, q if l is not None else None, c if idx is not None else None, M, T, _ws(M, T))
    torch.cuda.synchronize()
    assert (q[T:] == SENTINEL).all() and (c[T:] == SENTINEL).all(), "written past the end"
    if l is None:
        assert (q == SENTINEL).all(), "a null qsum pair was written"
    if idx is None:
        assert (c == SENTINEL).all(), "a null counts pair was written"
    return q[:T].cpu(), c[:T].cpu()


@pytest.mark.parametrize("M", M_VALUES)
@pytest.mark.parametrize("T", T_VALUES)
def test_codebook_usage_vs_float64(T, M):
    g = np.random.default_rng([T, M])
    for fam in ref.FAMILIES:
        l = ref.family(fam, M, T)
        rs, _ = _kl_fwd(l)
        idx = g.integers(0, T, size=M).astype(np.int32)
        ld, idd = torch.from_numpy(l).to(DEV), torch.from_numpy(idx).to(DEV)
        q, c = _run_usage(M, T, ld, rs, idd)
        err, bound = np.abs(q.double().numpy() - ref.qsum_spec(l)), ref.qsum_bound(l)
        assert np.isfinite(q.numpy()).all() and (err <= bound).all(), (fam, T, M, float(np.max(err / bound)))
        assert np.array_equal(c.numpy(), np.bincount(idx, minlength=T)), (fam, T, M)
        q2, c2 = _run_usage(M, T, ld, rs, idd)
        assert torch.equal(q2.view(torch.int32), q.view(torch.int32)) and torch.equal(c2, c)
        # either pair alone: the same values, the other output untouched
        q3, _ = _run_usage(M, T, ld, rs, None)
        _, c3 = _run_usage(M, T, None, None, idd)
        assert torch.equal(q3.view(torch.int32), q.view(torch.int32)) and torch.equal(c3, c), (fam, T, M)


@pytest.mark.parametrize("T", [64, 1032, 4096])
def test_codebook_usage_counts_are_exact(T):
    for M, idx in ((1030, np.full(1030, T - 3)),                       # every row picks one code
                   (2 * T + 5, np.arange(2 * T + 5) % T),               # index covers all T codes
                   (40000, np.random.default_rng(T).integers(0, T, 40000)),     # more rows than 512 slabs of 32: slabs grow
                   (7, np.array([0, T - 1, -1, T, 5, 5, 2 ** 30]))):    # values outside [0, T) are not counted
        idx = idx.astype(np.int32)
        _, c = _run_usage(M, T, None, None, torch.from_numpy(idx).to(DEV))
        ok = idx[(idx >= 0) & (idx < T)]
        assert np.array_equal(c.numpy(), np.bincount(ok, minlength=T)), (T, M)
        assert int(c.sum()) == len(ok)


def test_elbo_loss_is_one_rounding():
    g = np.random.default_rng(5)
    for _ in range(20):
        r, k, b = (np.float32(abs(v)) for v in g.standard_normal(3) * (0.1, 3.0, 5.0))
        rd, kd, out = (torch.tensor([v], dtype=torch.float32, device=DEV) for v in (r, k, 0.0))
        dh.elbo_loss(rd, kd, out, float(b))
        want = np.float32(np.float64(r) + np.float64(b) * np.float64(k))
        assert np.float32(out.item()).tobytes() == want.tobytes(), (r, k, b)
        out2 = torch.zeros_like(out)
        dh.elbo_loss(rd, kd, out2, 0.0, kl_weight_dev=torch.tensor([b], dtype=torch.float32, device=DEV))
        assert torch.equal(out2, out)


# ------------------------------------------------------------------ engine
SMALL = dict(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch_size=2)                     # the smallest VAE the kernels allow
EXAMPLE = dict(num_tokens=512, dimensions=32, convblocks=[[3, 64], [3, 128], [3, 256]], batch_size=1)     # configs/vae_example.json
SHAPES = [pytest.param(SMALL, id="small"), pytest.param(EXAMPLE, id="vae_example")]


def _sha(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _vae(shape, **kw):
    from src.vae_tf import DiscreteVAE
    vae = DiscreteVAE(use_bf16=True, **shape, **kw)
    vae.init_params(seed=4321)
    return vae


def _batch(vae, t=0):
    from oracle import vae_oracle as vo
    img = torch.from_numpy(vo.synthetic_images(vae.B, vae.H, seed=10 + t))
    u = torch.from_numpy(vo.synthetic_uniforms((vae.B, vae.grid, vae.grid, vae.num_tokens), seed=20 + t))
    return img, u


@pytest.fixture
def recorder():
    """the launch recorder of tools/launch_trace.py in place of the loaded library, for the duration of one test"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from launch_trace import Recorder
    real = dh.lib()
    rec = dh._lib = Recorder(real)
    try:
        yield rec
    finally:
        dh._lib = real


@pytest.mark.parametrize("shape", SHAPES)
def test_engine_keys_off_is_unchanged(shape, recorder):
    """kl_loss_weight = 0.0 is the model without the keyword: the same launches with the same arguments, and loss, gradients and
    weights after three steps equal bit for bit; no KL buffer exists"""
    runs = []
    for kw in ({}, dict(kl_loss_weight=0.0)):
        vae = _vae(shape, **kw)
        assert vae.rowstat is None and vae.loss_kl is None and vae._dyn.numel() == 3
        recorder.reset()
        losses = []
        for t in range(3):
            img, u = _batch(vae, t)
            losses.append(_sha(vae.train_step(img, 1e-3, noise=u, graph=False)))
        names = {v: k for k, v in recorder.table.items()}
        seq = [names[i] for i in recorder.sequence]
        assert not any("kl" in c or "usage" in c or "elbo" in c for c in seq)
        runs.append((seq, losses, _sha(vae.g), _sha(vae.p), _sha(vae.m), _sha(vae.v)))
        del vae
    assert runs[0][0] == runs[1][0], "launch sequence differs"
    assert runs[0][1:] == runs[1][1:]


@pytest.mark.parametrize("shape", SHAPES)
def test_engine_loss_and_gradient_with_kl(shape):
    """beta = 2: loss[0] is one fp32 rounding of loss_recon + beta_t loss_kl; loss_kl is the float64 KL of the engine's own logits
    inside the kernel bound; the dlogits buffer is the float64 formula on the engine's own dy, y_soft, logits inside the kernel
    bound (everything downstream of dlogits is existing, tested code) -- in train mode with a gradient and in eval mode"""
    vae = _vae(shape, kl_loss_weight=2.0)
    img, u = _batch(vae)
    for mode, temp in (("train", 1.0), ("eval", 0.5)):
        vae.mode = mode
        loss, _ = vae.forward(img, return_recon_loss=True, hard_gumbel=(mode == "train"), temperature=temp, noise=u)
        r, k = np.float64(vae.loss_recon.item()), np.float64(vae.loss_kl.item())
        assert np.float32(loss.item()).tobytes() == np.float32(r + 2.0 * k).tobytes(), (mode, loss.item(), r, k)
        assert np.float32(vae.loss.item()).tobytes() == np.float32(loss.item()).tobytes() and vae.kl_weight_t == 2.0
        l = vae.logits.cpu().numpy()
        assert abs(k - ref.kl_spec(l)["kl"]) <= ref.kl_bound(l), (mode, k, ref.kl_spec(l)["kl"])
        assert k > 0 and r > 0
    vae.mode = "train"
    vae.forward(img, return_recon_loss=True, hard_gumbel=True, temperature=0.5, noise=u, need_grad=True)
    vae.backward()
    torch.cuda.synchronize()
    l, dy, p = vae.logits.cpu().numpy(), vae.dy.float().cpu().numpy(), vae.y_soft.float().cpu().numpy()
    want, bound = ref.dlogits_from_terms(ref.bwd_terms(dy, p, l), 0.5, 2.0)
    err = np.abs(vae.dlogits.double().cpu().numpy() - want)
    assert (err <= bound).all(), (float(np.max(err / bound)), np.argwhere(err > bound)[:4].tolist())


@pytest.mark.parametrize("shape", SHAPES)
def test_engine_graph_equals_eager_under_the_ramp(shape):
    """three train_steps with kl_anneal_steps = 2 (beta_t = 0, beta / 2, beta): the replayed graph reads beta_t from device memory
    and equals the eager steps bit for bit in loss, the two loss terms, gradients, weights and Adam state"""
    runs = {}
    for mode in ("eager", "graph"):
        vae = _vae(shape, kl_loss_weight=2.0, kl_anneal_steps=2)
        out = []
        for t in range(3):
            img, u = _batch(vae, t)
            loss = vae.train_step(img, 1e-3, hard_gumbel=True, temperature=1.0 - 0.2 * t, noise=u, graph=(mode == "graph"))
            assert vae.kl_weight_t == (0.0, 1.0, 2.0)[t]
            out += [_sha(loss), _sha(vae.loss_recon), _sha(vae.loss_kl), _sha(vae.dlogits)]
        if mode == "graph":
            assert len(vae._graphs) == 1
        runs[mode] = out + [_sha(vae.g), _sha(vae.p), _sha(vae.m), _sha(vae.v)]
        del vae
    assert runs["eager"] == runs["graph"]


def test_engine_kl_term_lowers_the_kl():
    """beta = 5, soft Gumbel at temperature 1, fixed seeds (vae_kl_ref.SIGN_CASE: parameter seed 4321, learning rate 1e-3, one
    batch, noise seed 7 + step): loss_kl after 20 steps is below its value at step 0.  tests/test_vae_kl.py confirms on the CPU
    oracle, with the KL term added there in the test's own code, that the reference step does this for these seeds and this rate."""
    from oracle import vae_oracle as vo
    c = ref.SIGN_CASE
    vae = _vae(dict(num_tokens=c["num_tokens"], dimensions=c["dimensions"], convblocks=c["convblocks"], batch_size=c["batch"]),
               kl_loss_weight=c["beta"])
    img = torch.from_numpy(vo.synthetic_images(c["batch"], c["dimensions"], seed=c["image_seed"]))
    kls = []
    for t in range(c["steps"] + 1):
        u = torch.from_numpy(vo.synthetic_uniforms((c["batch"], vae.grid, vae.grid, c["num_tokens"]), seed=c["noise_seed"] + t))
        if t == c["steps"]:
            vae.forward(img, return_recon_loss=True, hard_gumbel=False, temperature=1.0, noise=u, need_grad=False)
        else:
            vae.train_step(img, c["lr"], hard_gumbel=False, temperature=1.0, noise=u)
        kls.append(vae.loss_kl.item())
    print("loss_kl per step:", kls, flush=True)
    assert kls[-1] < kls[0], kls


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("beta", [0.0, 2.0])
def test_engine_codebook_stats(shape, beta, recorder):
    """codebook_stats() after an eval forward is the host restatement from the engine's logits / index; with the weight off it runs
    dmi_codebook_kl_fwd itself; a train_step records no statistics launch (nothing of it is inside the captured graph)"""
    vae = _vae(shape, **({"kl_loss_weight": beta} if beta else {}))
    for t in range(3):
        img, u = _batch(vae, t)
        vae.train_step(img, 1e-3, noise=u)
    names = {v: k for k, v in recorder.table.items()}
    assert not any("usage" in names[i] for i in recorder.sequence)
    assert any("codebook_kl_fwd" in names[i] for i in recorder.sequence) == (beta > 0)
    vae.mode = "eval"
    img, u = _batch(vae, 9)
    vae.forward(img, return_recon_loss=True, hard_gumbel=True, temperature=1.0, noise=u, need_grad=False)
    recorder.reset()
    st = vae.codebook_stats()
    names = {v: k for k, v in recorder.table.items()}
    ran = [names[i].split("(")[0] for i in recorder.sequence]
    assert ran == (["codebook_usage"] if beta > 0 else ["codebook_kl_fwd", "codebook_usage"]), ran
    l, idx = vae.logits.cpu().numpy(), vae.index.cpu().numpy()
    want = ref.stats_spec(l, idx)
    assert abs(st["kl"] - want["kl"]) <= ref.kl_bound(l)
    assert st["codes_used"] == want["codes_used"] and st["codes_used_frac"] == want["codes_used_frac"]
    assert st["perplexity_hard"] == pytest.approx(want["perplexity_hard"], rel=1e-12)      # exact counts, float64 host arithmetic
    # perplexity_soft = exp(H(qsum / M)): |dH| <= sum_k |d qsum_k| / M * (|ln(qsum_k / M)| + 1) to first order; the host divides by
    # sum_k qsum_k, which is M within sum_k |d qsum_k|: twice the first-order term covers both
    M = l.shape[0]
    qs = ref.qsum_spec(l)
    dH = float((ref.qsum_bound(l) / M * (np.abs(np.log(np.maximum(qs / M, 1e-300))) + 1.0)).sum())
    assert abs(np.log(st["perplexity_soft"]) - np.log(want["perplexity_soft"])) <= 2.0 * dH + 1e-12, (st, want, dH)
    assert vae.codebook_stats() == st                    # a second call: the row statistics are reused, the same bits


@pytest.mark.parametrize("beta", [0.0, 2.0])
def test_engine_codebook_stats_follow_the_replayed_steps(beta):
    """on the captured-graph path a step is one replay and no Python forward(): codebook_stats() after every step must describe
    that step's logits / index, with the weight off (it runs dmi_codebook_kl_fwd itself, each time) and on (the replay ran it)"""
    vae = _vae(SMALL, **({"kl_loss_weight": beta} if beta else {}))
    seen = []
    for t in range(5):                 # eager warm step, capture + replay, then replays; other images every step
        img, u = _batch(vae, 30 + 7 * t)
        vae.train_step(img, 1e-2, noise=u, graph=True)
        st = vae.codebook_stats()
        l, idx = vae.logits.cpu().numpy(), vae.index.cpu().numpy()
        want = ref.stats_spec(l, idx)
        assert abs(st["kl"] - want["kl"]) <= ref.kl_bound(l), (t, st["kl"], want["kl"])
        assert st["codes_used"] == want["codes_used"]
        assert st["perplexity_hard"] == pytest.approx(want["perplexity_hard"], rel=1e-12)
        M = l.shape[0]
        qsum = vae._usage["qsum"].double().cpu().numpy()
        assert (np.abs(qsum - ref.qsum_spec(l)) <= ref.qsum_bound(l)).all(), (t, float(np.abs(qsum.sum() - M)))
        seen.append(want["kl"])
    assert len(vae._graphs) == 1 and len(set(seen)) == 5       # the steps did differ: a stale result would have been caught


# ------------------------------------------------------------------ model function
def _params(tmp_path, **over):
    from src.utils import fetch_model_params
    p = fetch_model_params("vae_example")
    p.update(dict(train_batch_size=2, eval_batch_size=2, model_path=str(tmp_path), convblocks=[[1, 64]], num_tokens=64,
                  steps_per_checkpoint=10 ** 6, dataset={"train_path": "synthetic", "eval_path": "synthetic", "image_size": 32}))
    p.update(over)
    return p


STAT_KEYS = {"loss_recon", "loss_kl", "kl_weight", "perplexity_soft", "perplexity_hard", "codes_used_frac"}


@pytest.mark.parametrize("keys", [dict(codebook_stats=True), dict(kl_loss_weight=2.0, kl_anneal_steps=4), {}], ids=["stats", "kl", "off"])
def test_model_fn_summaries_and_eval_metrics(tmp_path, keys, caplog):
    """with "codebook_stats" on or a weight > 0 the train host_call writes the six scalars next to loss and temperature and
    evaluation returns them next to _loss; with the keys unset neither changes; one line is logged about what is on"""
    import json
    import logging
    from oracle import vae_oracle as vo
    from src.model_fns_tf import vae_model_fn
    from src.utils import ModeKeys
    p = _params(tmp_path, **keys)
    img = torch.from_numpy(vo.synthetic_images(2, 32, seed=1))
    with caplog.at_level(logging.INFO, logger="dalle_mtf_amd"):
        for _ in range(3):
            spec = vae_model_fn(img, img, ModeKeys.TRAIN, p)
            step = spec.train_op()
    assert len([r for r in caplog.records if "KL term" in r.getMessage() or "codebook statistics" in r.getMessage()]) == (1 if keys else 0)
    fn, tensors = spec.host_call
    fn(step, **tensors)
    rec = json.loads(open(tmp_path / "summaries.jsonl").read().strip().splitlines()[-1])
    model = p["_vae_state_train"]["model"]
    assert STAT_KEYS <= set(rec) if keys else not (STAT_KEYS & set(rec)), rec
    ev = vae_model_fn(img, img, ModeKeys.EVAL, p)
    assert set(ev.eval_metrics) == ({"_loss"} | STAT_KEYS if keys else {"_loss"})
    if keys:
        m = ev.eval_metrics
        assert 1.0 <= m["perplexity_hard"] <= 64.0 and 1.0 <= m["perplexity_soft"] <= 64.0 + 1e-6 and 0.0 < m["codes_used_frac"] <= 1.0
        assert m["loss_kl"] >= 0.0 and rec["step"] == 3
        if "kl_loss_weight" in keys:
            assert rec["kl_weight"] == 2.0 * 2 / 4 and m["kl_weight"] == 2.0 * 3 / 4        # beta_t of step 2 (0-based) and of the eval at step 3
            assert np.float32(float(ev.loss)) == np.float32(np.float64(m["loss_recon"]) + np.float64(np.float32(m["kl_weight"])) * m["loss_kl"])
        else:
            assert m["kl_weight"] == 0.0 and m["loss_recon"] == float(ev.loss) and model.kl_weight == 0.0
