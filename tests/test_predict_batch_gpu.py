"""Generation and VAE decoding at the shipped predict batch (configs/dalle_coco.json: predict_batch_size 128).

At that batch the decode step leaves its B <= 32 form (LayerNorm fused into the products, dmi_ln_gemm_nt) for separate
dmi_layernorm_fwd launches and 128x128-tile dmi_gemm_nt products with M = B (a row tail for 32 < B < 128); the vae_coco decoder's
last residual pair holds 128 x 256 x 256 x 128 bf16 = 2 GiB activations, more than one buffer descriptor of the implicit
convolution kernels addresses; and the evaluation head writes 163 840 x 52 352 bf16 logits = 17 GB.  Every other generation test
runs at B <= 5 with toy dimensions.

A. the decode step above 32 rows against the full forward, graph against eager, every draw path against the others;
B. the vae_coco decoder / encoders / training step at B = 128 against the same images in B = 8 models;
C. the evaluation head's output rows beyond 2, 4 and 8 GiB against fp32 math, by direct call and at the forward's call site;
D. generate_dalle.py at dalle_coco dimensions and its default batch, end to end."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))


def _report(name, t0):
    torch.cuda.synchronize()
    print(f"{name}: {time.perf_counter() - t0:.1f} s, peak {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB", flush=True)


# ------------------------------------------------------------------------------------------------ A. decode above 32 rows
def _engine(B, **hp):
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    T, P, tv, iv = 16, 304, 60, 64
    cfg = do.DalleConfig(128, tv, iv, T, P, 2, 1)
    eng = DalleEngine(128, 2, 1, tv, iv, T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10, **hp))
    eng.load_reference_params(do.init_params(cfg, seed=9, perturb=0.05))
    toks = torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, T, tv, seed=1),
                                               do.synthetic_image_tokens(B, P, iv, seed=2), tv)).to(DEV)
    return eng, toks


POSITIONS = list(range(16 - 1, 16 + 70)) + [127, 128, 129, 255, 256, 318, 319]   # test_kv_cached_decode_equals_full_forward's


def _decode_vs_full(eng, toks, check_graph=True):
    """teacher-forced decode_step logits at POSITIONS, every batch row, against the full forward's; returns (worst, scale)"""
    B, S, tv, iv = eng.B, eng.S, eng.text_vocab_size, eng.image_vocab_size
    eng.forward(toks, need_grad=False)
    full = eng.z.view(B, S, eng.Vp)[:, :, tv:tv + iv].float().clone()
    worst = 0.0
    out = {}
    for i, p in enumerate(POSITIONS):
        z = eng.decode_step(toks[:, p].contiguous(), p)
        worst = max(worst, float((z - full[:, p]).abs().max()))
        out[p] = z.clone()
        if check_graph and (i % 7 == 0 or p > 100):   # replayed graph (steps >= 2) and eager launches: the same bits
            assert torch.equal(eng.decode_step(toks[:, p].contiguous(), p, graph=False), out[p]), p
    return worst, float(full.abs().max()), out


@pytest.mark.parametrize("B", [33, 40, 128])
def test_decode_step_above_32_rows(B):
    """B > 32: the unfused decode body (layernorm_fwd + tiled gemm_nt, M = B) against the full forward at every row, and every
    sampling path against the others.  Measured on MI355X: max |dlogit| 0.0063 (B = 33, 40) and 0.0071 (B = 128) of a 1.05 logit
    range; about 1 s and at most 0.6 GiB per batch size."""
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    eng, toks = _engine(B)
    T, P, S, tv, iv = eng.T, eng.S - eng.T, eng.S, eng.text_vocab_size, eng.image_vocab_size
    worst, scale, _ = _decode_vs_full(eng, toks)
    print(f"B = {B}: decode vs full forward max |dlogit| {worst} of {scale}")
    assert worst <= 2.5e-2 * scale, (worst, scale)
    assert eng._dec["graphs"].get(False) is not None
    text = toks[:, :T].contiguous()
    # greedy: the three cached paths agree bit for bit; the plain sampler up to near-ties of the full forward's logits
    a = eng.sample_image_tokens(text, temperature=0.0)
    assert torch.equal(a, eng.sample_image_tokens(text, temperature=0.0, fused_sampling=False))
    assert torch.equal(a, eng.sample_image_tokens(text, temperature=0.0, decode_graph=False))
    b = eng.sample_image_tokens(text, temperature=0.0, kv_cache=False)
    for i in range(B):
        bad = (a[i] != b[i]).nonzero()
        if len(bad) == 0:
            continue
        f = int(bad[0])
        seq = torch.cat([text[i], b[i, :f].to(torch.int32) + tv, torch.full((P - f,), tv, dtype=torch.int32, device=DEV)])
        eng.forward(seq.repeat(B, 1), need_grad=False)
        top2 = eng.z.view(B, S, eng.Vp)[0, T + f - 1, tv:tv + iv].float().topk(2).values
        assert float(top2[0] - top2[1]) <= 2 * worst + 1e-3, (i, f, float(top2[0] - top2[1]), worst)
    # top-k and top-p: fused graph draw = host-launched draw = eager decode, bit for bit; rows draw different noise
    for kw in (dict(temperature=1.0, top_k=8, seed=3), dict(temperature=1.0, top_p=0.9, seed=5)):
        s = eng.sample_image_tokens(text, **kw)
        assert int(s.min()) >= 0 and int(s.max()) < iv
        assert torch.equal(s, eng.sample_image_tokens(text, **kw, fused_sampling=False)), kw
        assert torch.equal(s, eng.sample_image_tokens(text, **kw, decode_graph=False)), kw
        assert not torch.equal(s[0], s[B - 1])
        # completion of the sample's prefix reproduces the sample
        for k in (1, 17, P - 1):
            c = eng.sample_image_tokens(text, image_prefix=s[:, :k], **kw)
            assert torch.equal(c, s), (kw, k, (c != s).nonzero()[:3])
    # the model's score of its samples: the sum of decode-step log-softmax at the drawn tokens
    toks_lp, lp = eng.sample_image_tokens(text, temperature=1.0, top_p=0.9, seed=7, return_logprobs=True)
    full = torch.cat([text, toks_lp.to(torch.int32) + tv], 1)
    eng._prefill(full)
    want = torch.zeros(B, dtype=torch.float64)
    for pos in range(T - 1, S - 1):
        z = eng.decode_step(full[:, pos].contiguous(), pos).double().cpu()
        want += torch.log_softmax(z, -1)[torch.arange(B), toks_lp[:, pos - T + 1].cpu().long()]
    got = lp.double().cpu()
    assert bool(((got - want).abs() <= 1e-4 * want.abs()).all()), (got - want).abs().max()
    _report(f"test_decode_step_above_32_rows[{B}]", t0)


def test_unfused_decode_equals_fused_decode_at_3_rows():
    """decode_fuse_ln=False at B = 3 (the B > 32 body on a batch the fused body also serves): both against the full forward, and
    against each other on the same inputs, within the full-forward bound.  Measured on MI355X: both bodies 0.0052 from the full
    forward, identical to each other (0.0); 0.25 s."""
    eng_u, toks = _engine(3, decode_fuse_ln=False)
    eng_f, _ = _engine(3)
    wu, scale, zu = _decode_vs_full(eng_u, toks)
    wf, _, zf = _decode_vs_full(eng_f, toks, check_graph=False)
    diff = max(float((zu[p] - zf[p]).abs().max()) for p in POSITIONS)
    print(f"B = 3: unfused {wu}, fused {wf}, unfused vs fused {diff} of {scale}")
    assert wu <= 2.5e-2 * scale and wf <= 2.5e-2 * scale and diff <= 2.5e-2 * scale, (wu, wf, diff, scale)
    text = toks[:, :eng_u.T].contiguous()
    for kw in (dict(temperature=1.0, top_k=8, seed=3), dict(temperature=1.0, top_p=0.9, seed=5)):
        s = eng_u.sample_image_tokens(text, **kw)
        assert torch.equal(s, eng_u.sample_image_tokens(text, **kw, decode_graph=False))
        assert torch.equal(s, eng_u.sample_image_tokens(text, image_prefix=s[:, :17], **kw))


# ------------------------------------------------------------------------------------------------ B. vae_coco at B = 128
def _coco_vae(B, P, **kw):
    from src.vae_tf import DiscreteVAE
    p = json.load(open(os.path.join(ROOT, "configs", "vae_coco.json")))
    v = DiscreteVAE(num_tokens=p["num_tokens"], dimensions=p["dataset"]["image_size"], convblocks=p["convblocks"],
                    batch_size=B, use_bf16=True, **kw)
    v.load_reference_params(P)
    return v


def _coco_params(seed=11):
    from oracle import vae_oracle as vo
    p = json.load(open(os.path.join(ROOT, "configs", "vae_coco.json")))
    cfg = vo.VaeConfig(num_tokens=p["num_tokens"], dimensions=p["dataset"]["image_size"], convblocks=p["convblocks"])
    return cfg, vo.init_params(cfg, seed=seed, bias_perturb=0.05)


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_vae_coco_decode_and_encode_at_batch_128_equal_batch_8():
    """128 images of 256 x 256: the decoder's 256 x 256 x 128 residual pair is 2 GiB per activation (dmi_conv_gemm_nt used to
    refuse it: one buffer descriptor of < 2 GiB; the batch now runs in whole-image chunks).  No layer couples images and every
    kernel computes an output row independently of M, so each image of the B = 128 decode / encode equals the same image in a
    B = 8 model bit for bit -- for the bf16 decoder, the bf16 encoder's logits and the fp32 tokenising encoder's logits.
    Measured on MI355X: bit-identical everywhere; 2.4 s, peak 57.7 GiB (the B = 128 model)."""
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    cfg, P = _coco_params()
    B, b = 128, 8
    g = torch.Generator(device=DEV).manual_seed(3)
    tokens = torch.randint(0, cfg.num_tokens, (B, cfg.grid * cfg.grid), generator=g, device=DEV, dtype=torch.int32)
    img = torch.rand(B, 256, 256, 3, generator=g, device=DEV) * 2 - 1
    big = _coco_vae(B, P, mode="predict")
    dec = big.decode_tokens(tokens).clone()
    lg = big.forward(img, return_logits=True).clone()
    big.fp32_tokens = True
    lg32 = big.forward(img, return_logits=True).clone()
    _report("vae_coco B = 128 decode + both encoders", t0)
    del big
    _free()
    small = _coco_vae(b, P, mode="predict")
    assert bool(torch.isfinite(dec).all()) and float(dec.abs().max()) > 0
    for i in range(0, B, b):
        d8 = small.decode_tokens(tokens[i:i + b].contiguous())
        assert torch.equal(d8, dec[i:i + b]), (i, float((d8 - dec[i:i + b]).abs().max()))
        l8 = small.forward(img[i:i + b].contiguous(), return_logits=True)
        assert torch.equal(l8, lg[i:i + b]), (i, float((l8 - lg[i:i + b]).abs().max()))
    small.fp32_tokens = True
    for i in range(0, B, b):
        l8 = small.forward(img[i:i + b].contiguous(), return_logits=True)
        assert torch.equal(l8, lg32[i:i + b]), (i, float((l8 - lg32[i:i + b]).abs().max()))
    del small
    _free()
    _report("test_vae_coco_decode_and_encode_at_batch_128_equal_batch_8", t0)


def test_vae_coco_batch_128_gradient_is_the_mean_of_sixteen_batch_8_gradients():
    """One training step at B = 128 (the config's train_batch_size; every 256 x 256 convolution's forward, input gradient and weight
    gradient runs in whole-image chunks): the gradient is the mean of the sixteen B = 8 gradients, as
    test_vae_coco_benchmark_batch_gradient_is_the_mean_of_the_two_image_gradients checks at B = 16.  Soft Gumbel.  Measured on
    MI355X: worst tensor 2.3e-6 relative L2 (decoder/block_2/layer_0/conv_upsample/kernel); 3.3 s, peak 53.9 GiB."""
    from oracle import vae_oracle as vo
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    cfg, P = _coco_params()
    B, b = 128, 8
    g = torch.Generator(device=DEV).manual_seed(7)
    img = torch.rand(B, 256, 256, 3, generator=g, device=DEV) * 2 - 1
    u = torch.rand(B, cfg.grid, cfg.grid, cfg.num_tokens, generator=g, device=DEV).clamp_(1e-6, 1.0 - 1e-6)

    def grads(vae, x, n):
        vae.forward(x, return_recon_loss=True, hard_gumbel=False, temperature=1.0, noise=n, need_grad=True)
        vae.backward()
        torch.cuda.synchronize()
        return {k: v.astype(np.float64) for k, v in vae.export_reference(vae.g).items()}
    big = _coco_vae(B, P)
    gb = grads(big, img, u)
    _report("vae_coco B = 128 training step", t0)
    del big
    _free()
    small = _coco_vae(b, P)
    acc = None
    for i in range(0, B, b):
        g8 = grads(small, img[i:i + b].contiguous(), u[i:i + b].contiguous())
        acc = g8 if acc is None else {k: acc[k] + g8[k] for k in acc}
    del small
    _free()
    mean = {k: v / (B // b) for k, v in acc.items()}
    table = {k: float(np.linalg.norm(gb[k] - mean[k]) / max(np.linalg.norm(mean[k]), 1e-30)) for k in gb}
    worst = max(table.items(), key=lambda t: t[1])
    print("vae_coco B = 128 gradient vs the mean of sixteen B = 8 gradients: worst tensor", worst, flush=True)
    assert all(np.isfinite(v).all() for v in gb.values())
    assert worst[1] <= 1e-4, worst
    _report("test_vae_coco_batch_128_gradient_is_the_mean_of_sixteen_batch_8_gradients", t0)


def test_conv_gemm_nt_on_whole_image_pieces_equals_one_launch():
    """What the batch split relies on: launches over whole-image pieces (here 9 + 7 of 16 images of 256 x 256 x 64, with bias and
    residual epilogue) give the bits of one launch over the batch; a single image of 2 GiB or more is still refused, by the
    forward and by the weight gradient."""
    import dalle_hip as dh
    from src.vae_tf.models import TAPS3
    B, H, C, N = 16, 256, 64, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    x = (torch.randn(B * H * H, C, generator=g, device=DEV)).to(torch.bfloat16)
    Wt = (torch.randn(N, 9 * C, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g, device=DEV) * 0.1).to(torch.bfloat16)
    res = torch.randn(B * H * H, N, generator=g, device=DEV).to(torch.bfloat16)
    out = torch.empty(B * H * H, N, dtype=torch.bfloat16, device=DEV)
    dh.conv_gemm_nt(x, B, H, H, C, H, H, 1, TAPS3, Wt, 9 * C, out, N, N, dh.GEMM_BIAS | dh.GEMM_RESIDUAL, bias=bias, residual=res)
    part = torch.empty_like(out)
    r = 9 * H * H
    dh.conv_gemm_nt(x[:r], 9, H, H, C, H, H, 1, TAPS3, Wt, 9 * C, part[:r], N, N, dh.GEMM_BIAS | dh.GEMM_RESIDUAL, bias=bias,
                    residual=res[:r])
    dh.conv_gemm_nt(x[r:], 7, H, H, C, H, H, 1, TAPS3, Wt, 9 * C, part[r:], N, N, dh.GEMM_BIAS | dh.GEMM_RESIDUAL, bias=bias,
                    residual=res[r:])
    assert torch.equal(out, part)
    del x, res, out, part
    # one image of 4096 x 4096 x 64 = 2 GiB cannot be split: both kernels refuse it (buffers of the full size, so that the
    # calls stay in bounds whatever the guard does)
    big = torch.zeros(4096 * 4096, C, dtype=torch.bfloat16, device=DEV)
    big_out = torch.zeros(4096 * 4096, N, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(dh.DalleHipError, match="too large"):
        dh.conv_gemm_nt(big, 1, 4096, 4096, C, 4096, 4096, 1, TAPS3, Wt, 9 * C, big_out, N, N)
    dW = torch.zeros(9 * C, N, dtype=torch.float32, device=DEV)
    w = torch.empty(max(dh.conv_wgrad_tn_workspace_bytes(4096 * 4096, 9 * C, N), 256), dtype=torch.uint8, device=DEV)
    with pytest.raises(dh.DalleHipError, match="too large"):
        dh.conv_wgrad_tn(big, 1, 4096, 4096, C, 4096, 4096, 1, TAPS3, big_out, N, N, dW, w)
    del big, big_out
    _free()


def test_conv_wgrad_tn_chunked_batch_vs_float64():
    """The weight gradient of vae_coco's 256 x 256 x 128 residual conv at B = 128: x is 2 GiB, so the batch runs as two launches
    (127 + 1 images, the most that fit one descriptor) whose slabs one reduce adds.  x is zero except in images 0, 126 (the
    first chunk's last) and 127 (the second chunk), dY is random everywhere: dW must equal float64 math over those three
    images, and dbias (the column sums of all of dY) float64 sums -- a dropped chunk or a wrong image offset fails."""
    import dalle_hip as dh
    from src.vae_tf.models import TAPS3
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    B, H, C, N = 128, 256, 128, 128
    px = H * H
    g = torch.Generator(device=DEV).manual_seed(17)
    hot = [0, 126, 127]
    x = torch.zeros(B * px, C, dtype=torch.bfloat16, device=DEV)
    for i in hot:
        x[i * px:(i + 1) * px] = torch.randn(px, C, generator=g, device=DEV).to(torch.bfloat16)
    dY = torch.randn(B * px, N, generator=g, device=DEV, dtype=torch.bfloat16)
    dW = torch.full((9 * C, N), float("nan"), dtype=torch.float32, device=DEV)
    db = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
    w = torch.empty(dh.conv_wgrad_tn_workspace_bytes(B * px, 9 * C, N), dtype=torch.uint8, device=DEV)
    dh.conv_wgrad_tn(x, B, H, H, C, H, H, 1, TAPS3, dY, N, N, dW, w, dbias=db)
    torch.cuda.synchronize()
    ref = torch.zeros(9 * C, N, dtype=torch.float64, device=DEV)
    for i in hot:
        xp = torch.zeros(H + 2, H + 2, C, dtype=torch.float64, device=DEV)
        xp[1:H + 1, 1:H + 1] = x[i * px:(i + 1) * px].view(H, H, C).double()
        dyi = dY[i * px:(i + 1) * px].double()
        for t, (ty, tx) in enumerate(TAPS3):      # out[(oy, ox)] reads x[oy + ty, ox + tx]
            ref[t * C:(t + 1) * C] += xp[1 + ty:1 + ty + H, 1 + tx:1 + tx + H].reshape(px, C).t() @ dyi
    refb = torch.zeros(N, dtype=torch.float64, device=DEV)
    for r0 in range(0, B * px, 1 << 20):
        refb += dY[r0:r0 + (1 << 20)].double().sum(0)
    for got, want, what in ((dW, ref, "dW"), (db, refb, "dbias")):
        err = (got.double() - want).abs()
        bad = ~(err <= 1e-5 * want.abs() + 1e-5 * float(want.abs().max()))
        assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float(want.abs().max()))
    del x, dY, w
    _free()
    _report("test_conv_wgrad_tn_chunked_batch_vs_float64", t0)


# ------------------------------------------------------------------------------------------------ C. head output beyond 4 GiB
M_HEAD, N_HEAD, K_HEAD = 163840, 52352, 1024          # dalle_coco at B = 128: 128 x 1280 rows, Vp = 50258 + 2048 padded


def _boundary_rows(M, N):
    row_bytes = N * 2
    rows = {0, M - 2, M - 1}
    for gib in (2, 4, 8, 16):
        r = (gib << 30) // row_bytes
        rows.update(x for x in (r - 1, r, r + 1) if 0 <= x < M)
    return sorted(rows)


def _check_head_rows(z, X, Wt, bias, rows, what):
    idx = torch.tensor(rows, device=DEV)
    ref = X[idx].double() @ Wt.double().t() + bias.double()
    got = z[idx].double()
    err = (got - ref).abs()
    tol = 2.0 ** -8 * ref.abs() + 1e-3 * float(ref.abs().max())      # bf16 rounding of the result + fp32 accumulation order
    assert bool(torch.isfinite(ref).all()), what
    bad = ~(err <= tol)        # a row left unwritten keeps the NaN sentinel: NaN compares false, so it counts as bad here
    assert not bool(bad.any()), (what, [rows[i] for i in bad.any(1).nonzero().flatten().tolist()][:8], float(err.max()))


def test_head_gemm_output_rows_beyond_4GiB():
    """dh.gemm_nt with GEMM_BIAS at the dalle_coco evaluation head at B = 128: C = 163 840 x 52 352 bf16 = 17.2 GB, so output rows
    lie past 2, 4 and 8 GiB (32-bit byte offsets wrap at 4 GiB, 32-bit element offsets at 8 GiB; the last row ends just below
    16 GiB).  Automatic kernel choice; rows on each side of every boundary against float64 math.  Measured on MI355X: 0.25 s,
    peak 16.9 GiB."""
    import dalle_hip as dh
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    M, N, K = M_HEAD, N_HEAD, K_HEAD
    g = torch.Generator(device=DEV).manual_seed(13)
    X = (torch.randn(M, K, generator=g, device=DEV) * 0.5).to(torch.bfloat16)
    Wt = (torch.randn(N, K, generator=g, device=DEV) * 0.05).to(torch.bfloat16)
    bias = (torch.randn(N, generator=g, device=DEV) * 0.1).to(torch.bfloat16)
    z = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=DEV)
    dh.gemm_nt(X, K, Wt, K, z, N, M, N, K, dh.GEMM_BIAS, bias=bias)
    torch.cuda.synchronize()
    rows = _boundary_rows(M, N)
    _check_head_rows(z, X, Wt, bias, rows, "gemm_nt head")
    tail = z[M - 64:]
    assert not bool(torch.isnan(tail.float()).any())
    del z
    _free()
    _report("test_head_gemm_output_rows_beyond_4GiB", t0)


def test_eval_forward_head_rows_beyond_4GiB():
    """The same product at its call site: DalleEngine.forward(need_grad=False) at dalle_coco dimensions (one layer: the head does
    not depend on depth), B = 128.  The logits of boundary rows against float64 math on the head's own input (xnf).  Measured on
    MI355X: 1.0 s, peak 30.2 GiB."""
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    t0 = time.perf_counter()
    torch.cuda.reset_peak_memory_stats()
    d, H, tv, iv, T, P, B = 1024, 8, 50258, 2048, 256, 1024, 128
    eng = DalleEngine(d, 1, H, tv, iv, T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10, recompute_grad=True))
    cfg = do.DalleConfig(d, tv, iv, T, P, 1, H)
    eng.load_reference_params(do.init_params(cfg, seed=3, perturb=0.05))
    toks = torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, T, tv, seed=1),
                                               do.synthetic_image_tokens(B, P, iv, seed=2), tv)).to(DEV)
    eng.z.fill_(float("nan"))
    eng.forward(toks, need_grad=False)
    torch.cuda.synchronize()
    assert eng.M == M_HEAD and eng.Vp >= tv + iv
    Wt, bias = eng.tview("to_logits/linear_out/kernel"), eng._w("to_logits/linear_out/bias")
    z = eng.z.view(eng.M, eng.Vp)
    rows = _boundary_rows(eng.M, eng.Vp)
    _check_head_rows(z, eng.xnf, Wt, bias, rows, "eval forward head")
    _report("test_eval_forward_head_rows_beyond_4GiB", t0)
    del eng, z
    _free()


# ------------------------------------------------------------------------------------------------ D. the documented command
def test_generate_cli_at_dalle_coco_default_batch(tmp_path):
    """README: generate_dalle.py --model dalle_coco --from-eval 32 --samples-per-caption 4 at the config's predict batch (128): random
    weights (no checkpoint, allow_random_vae), synthetic eval captions.  One batch of 128 rows sampled on the 12-layer model and
    decoded by the vae_coco decoder at B = 128 (before the conv kernels split their batch, decode_tokens raised on the 2-GiB
    activation).  Measured on MI355X: 10 s for the child process, peak 99 GiB in it."""
    cfg = json.load(open(os.path.join(ROOT, "configs", "dalle_coco.json")))
    cfg.update(allow_random_vae=True, model_path=str(tmp_path / "no_run"))
    vae = json.load(open(os.path.join(ROOT, "configs", "vae_coco.json")))
    vae.update(model_path=str(tmp_path / "no_vae_run"))
    json.dump(vae, open(tmp_path / "vae.json", "w"))
    cfg["vae_model"] = str(tmp_path / "vae.json")
    json.dump(cfg, open(tmp_path / "coco.json", "w"))
    out = tmp_path / "out"
    # the CLI in a child process; the child reports its peak device memory after generate() returns
    code = ("import runpy, sys, torch; sys.argv = sys.argv[1:]; runpy.run_path(sys.argv[0], run_name='__main__'); "
            "print('peak_gib', torch.cuda.max_memory_allocated() / 2**30)")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "generate_dalle.py"), "--model", str(tmp_path / "coco.json"),
                        "--from-eval", "32", "--samples-per-caption", "4", "--out", str(out)],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    print(f"generate_dalle.py at dalle_coco, B = 128: {time.perf_counter() - t0:.1f} s;", r.stdout.strip().splitlines()[-1])
    info = json.load(open(out / "generate.json"))
    assert info["batch"] == 128 and info["rows"] == 128 and info["batches"] == 1 and info["images_written"] == 128
    toks = np.load(out / "tokens.npy")
    lp = np.load(out / "logprob.npy")
    assert toks.shape == (128, 1024) and toks.dtype == np.int32 and toks.min() >= 0 and toks.max() < 2048
    assert lp.shape == (128,) and np.isfinite(lp).all() and (lp < 0).all()
    pngs = sorted(f for f in os.listdir(out) if f.endswith(".png"))
    assert len(pngs) == 128 and "0_0.png" in pngs and "31_3.png" in pngs
    from PIL import Image
    im = np.asarray(Image.open(out / "31_3.png"))
    assert im.shape == (256, 256, 3) and im.dtype == np.uint8
