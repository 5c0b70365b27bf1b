"""The pointwise and re-layout kernels of the discrete-VAE path (dalle-mtf_amd/csrc/vae.hip) against the float64 restatements of
tests/vae_kernels_ref.py, on the kernel's own fp32 / bf16 inputs: Gumbel-softmax forward and backward at every NC instantiation and
on both sides of each boundary, at the annealed temperatures vae_coco trains at; the MSE loss and its gradient; and bit-exact checks
of add_f32, pad / unpad, pixel_interleave, weight_gather and weight_gather_batch (hand-built tables and the one DiscreteVAE builds
for vae_coco).  The whole-model regimes (T = 0.05 soft, hard Gumbel) are in tests/test_vae_coco_parity_gpu.py."""
import json
import os

import numpy as np
import pytest
import torch

import dalle_hip as dh
import vae_kernels_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U_MIN, U_MAX = np.float32(1e-9), np.float32(0.99999994)    # the engine's uniform floor; the largest fp32 below 1

# every gumbel_fwd_kernel<NC> instantiation (NC = 1/2/4/8 for T <= 512/1024/2048/4096) and both sides of each boundary
T_VALUES = [8, 504, 512, 520, 1024, 1032, 2048, 2056, 4096]
TEMPS = [1.0, 0.5, 0.05]       # 0.05: vae_coco's temperature after its 25k-step anneal


def _bf16_ulp(x):
    """one bf16 ulp at |x| (7 explicit mantissa bits); the ulp of the smallest normal below it"""
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126)))
    return 2.0 ** (e - 7)


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _big_m(T):
    return 4097 if T <= 1032 else 1025          # 4k + 1 rows: the last block runs one wave of four


def _gumbel_inputs(M, T, seed):
    g = np.random.default_rng(seed)
    l = (g.standard_normal((M, T)) * 2.0).astype(np.float32)
    u = np.clip(g.uniform(1e-9, 1.0, (M, T)).astype(np.float32), U_MIN, U_MAX)
    return l, u


SENTINEL = -12345      # bf16 bit pattern 0xCFC7 (about -6.7e9): never a probability, a softmax gradient or a weight


def _gumbel_fwd(l, u, T, temp, hard, temp_dev=None, extra=4):
    """runs the kernel on M rows of buffers with `extra` more rows, which must stay untouched"""
    M = l.shape[0]
    y = torch.full((M + extra, T), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    ys = torch.full((M + extra, T), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    idx = torch.full((M + extra,), -7, dtype=torch.int32, device=DEV)
    dh.gumbel_softmax_fwd(torch.from_numpy(l).to(DEV), torch.from_numpy(u).to(DEV), y, ys, idx, M, T, temp, hard,
                          temperature_dev=temp_dev)
    torch.cuda.synchronize()
    assert (_bits(y[M:]) == SENTINEL).all() and (_bits(ys[M:]) == SENTINEL).all() and (idx[M:] == -7).all(), "rows >= M written"
    return y[:M].cpu(), ys[:M].cpu(), idx[:M].cpu()


def _z_error_bound(l, u, temp):
    """bound on |z_fp32 - z| per element.  The kernel computes g = -logf(-logf(u)) (each logf within 2 ulp: the inner one's
    relative error becomes an absolute error of the outer one), then (l + g) * fl(1/T): the add, the fp32 reciprocal and the
    multiply round once each.  That is at most 7 * 2^-24 * (|l| + |g| + 1) / T; stated as 2^-21 (|l| + |g| + 1) / T."""
    g = ref.gumbel_noise(u)
    return 2.0 ** -21 * (np.abs(l.astype(np.float64)) + np.abs(g) + 1.0) / float(np.float32(temp))


def _check_fwd(l, u, T, temp, hard, y, ys, idx, tag):
    y_r, p_r, _ = ref.gumbel_fwd(l, u, temp, hard)
    ysd = ys.double().numpy()
    # y_soft: softmax of z = (l + g) / T rounded to bf16.  fp32 z error is <= 2^-21 (|l| + |g| + 1) / T (above), i.e. a few 1e-6
    # relative on p; __expf and the 1/sum add a few fp32 ulp: far inside the bf16 rounding, so one bf16 ulp of p bounds the error
    # (plus 2^-126 for probabilities in the subnormal range).
    err = np.abs(ysd - p_r)
    bound = _bf16_ulp(p_r) + 2.0 ** -126
    bad = ~(err <= bound)
    assert not bad.any(), (tag, "y_soft", int(bad.sum()), float(err.max()), np.argwhere(bad)[:4].tolist())
    z = ref.gumbel_z(l, u, temp)
    am, gap = ref.top2_gap(z)
    ez = _z_error_bound(l, u, temp).max(axis=-1)
    decided = gap > 2.0 * ez        # beyond the fp32 rounding of both z values, the kernel's arg-max is the float64 one
    assert decided.mean() >= 0.99, (tag, float(decided.mean()))
    idn = idx.numpy()
    assert np.array_equal(idn[decided], am[decided]), (tag, "index", np.argwhere(idn[decided] != am[decided])[:4].tolist())
    assert ((idn >= 0) & (idn < T)).all()
    if hard:
        yd = y.double().numpy()
        onehot = np.zeros_like(yd)
        onehot[np.arange(yd.shape[0]), idn] = 1.0
        assert np.array_equal(yd, onehot), (tag, "y is not one-hot at index")
    else:
        assert torch.equal(_bits(y), _bits(ys)), (tag, "soft y != y_soft")
    normal = p_r >= 2.0 ** -126
    return float((err[normal] / _bf16_ulp(p_r[normal])).max())


REPORT = {}


@pytest.mark.parametrize("T", T_VALUES)
def test_gumbel_fwd_vs_float64(T):
    Mb = _big_m(T)
    l, u = _gumbel_inputs(Mb, T, seed=T)
    worst = 0.0
    for temp in TEMPS:
        tdev = torch.tensor([temp], dtype=torch.float32, device=DEV)
        for hard in (False, True):
            y, ys, idx = _gumbel_fwd(l, u, T, temp, hard)
            worst = max(worst, _check_fwd(l, u, T, temp, hard, y, ys, idx, (T, temp, hard, Mb)))
            if hard:
                assert torch.equal(_bits(ys), _bits(ys_soft_mode)) and torch.equal(idx, idx_soft_mode)
            else:
                ys_soft_mode, idx_soft_mode = ys, idx
            # the graph-step path (1/T from device memory) is the host-temperature path bit for bit
            y2, ys2, idx2 = _gumbel_fwd(l, u, T, temp, hard, temp_dev=tdev)
            assert torch.equal(_bits(y2), _bits(y)) and torch.equal(_bits(ys2), _bits(ys)) and torch.equal(idx2, idx), (T, temp, hard)
        for M in (1, 3, 5):             # a block with 3, 1 and 3 idle waves
            for hard in (False, True):
                y, ys, idx = _gumbel_fwd(l[:M].copy(), u[:M].copy(), T, temp, hard)
                _check_fwd(l[:M], u[:M], T, temp, hard, y, ys, idx, (T, temp, hard, M))
    REPORT[f"fwd_T{T}"] = dict(worst_y_soft_err_in_bf16_ulp=worst)
    print("gumbel fwd T", T, "worst |y_soft - p| in bf16 ulp of p (normal range):", worst, flush=True)


def _tie_pairs(T):
    """column pairs with identical z: same lane and chunk, neighbouring lanes, far lanes, same lane in different NC chunks,
    different NC chunks"""
    cand = [(3, 5), (0, 7), (3, 8 * 17 + 2), (8, 8 * 63 + 1), (3, 512 + 3), (3, T - 8), (T - 16, T - 1), (520, 1040 + 7),
            (8, 8 * 64 * 7 + 4)]
    return sorted({(a, b) for a, b in cand if 0 <= a < b < T})


@pytest.mark.parametrize("T", T_VALUES)
def test_gumbel_fwd_exact_ties_take_the_lower_index(T):
    pairs = _tie_pairs(T)
    l, u = _gumbel_inputs(len(pairs), T, seed=100 + T)
    for r, (a, b) in enumerate(pairs):
        l[r, a] = l[r, b] = 60.0         # above every other l + g (|l| < 15, g < 17)
        u[r, a] = u[r, b] = 0.5
    for temp in TEMPS:
        for hard in (False, True):
            y, ys, idx = _gumbel_fwd(l, u, T, temp, hard)
            for r, (a, b) in enumerate(pairs):
                assert int(idx[r]) == a, (T, temp, hard, (a, b), int(idx[r]))     # tf.argmax / torch.argmax: the first maximum
                assert ys[r, a].item() == ys[r, b].item()
                if hard:
                    yr = y[r].float()
                    assert yr[a] == 1.0 and float(yr.sum()) == 1.0, (T, temp, (a, b))
    assert torch.argmax(torch.tensor([0.0, 1.0, 1.0])) == 1     # the convention the kernel follows


@pytest.mark.parametrize("T", [512, 2048, 4096])
def test_gumbel_fwd_extreme_uniforms(T):
    """uniforms at the engine's floor 1e-9 (g = -3.03) and at 0.99999994 (g = +16.6), whole rows and mixed"""
    M = 8
    l, u = _gumbel_inputs(M, T, seed=7)
    u[0], u[1] = U_MIN, U_MAX
    u[2, ::2], u[2, 1::2] = U_MIN, U_MAX
    u[3, ::3] = U_MAX
    u[4, ::5] = U_MIN
    for temp in TEMPS:
        for hard in (False, True):
            y, ys, idx = _gumbel_fwd(l, u, T, temp, hard)
            assert torch.isfinite(ys.float()).all() and torch.isfinite(y.float()).all(), (T, temp, hard)
            _check_fwd(l, u, T, temp, hard, y, ys, idx, ("extreme", T, temp, hard))


def _bwd(dy, ys, T, temp, temp_dev=None, extra=4):
    M = dy.shape[0]
    out = torch.full((M + extra, T), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    dh.gumbel_softmax_bwd(dy.to(DEV), ys.to(DEV), out, M, T, temp, temperature_dev=temp_dev)
    torch.cuda.synchronize()
    assert (_bits(out[M:]) == SENTINEL).all(), "rows >= M written"
    return out[:M].cpu()


@pytest.mark.parametrize("T", T_VALUES)
def test_gumbel_bwd_vs_float64(T):
    """dlogits = (1/T) p (dy - sum_j dy_j p_j) on the kernel's own bf16 y_soft and a bf16 dy.  Error model: the bf16 x bf16
    products are exact in fp32; each lane sums T/64 of them, then 6 butterfly levels: |dot error| <= (T/64 + 6) 2^-24 S,
    S = sum |dy_j p_j|.  (dy_k - dot), the two multiplies and the fp32 1/T round once each: <= 4 * 2^-24 (|dy_k| + |dot|)
    relative to p_k / T.  Then the bf16 output rounds to nearest: half an ulp of the fp32 value."""
    Mb = _big_m(T)
    l, u = _gumbel_inputs(Mb, T, seed=3 * T + 1)
    g = torch.Generator().manual_seed(T)
    dy = (torch.randn(Mb, T, generator=g) * 0.01).to(torch.bfloat16)
    worst = 0.0
    for temp in TEMPS:
        _, ys, _ = _gumbel_fwd(l, u, T, temp, False)
        dl = _bwd(dy, ys, T, temp)
        r = ref.gumbel_bwd(dy.double().numpy(), ys.double().numpy(), temp)
        p, a = ys.double().numpy(), dy.double().numpy()
        S = np.abs(a * p).sum(axis=-1, keepdims=True)
        dot = (a * p).sum(axis=-1, keepdims=True)
        it = 1.0 / float(np.float32(temp))
        E = it * p * 2.0 ** -24 * ((T / 64 + 8) * S + 4 * (np.abs(a) + np.abs(dot)))
        bound = E + 0.5 * _bf16_ulp(np.abs(r) + E) + it * 2.0 ** -126
        err = np.abs(dl.double().numpy() - r)
        bad = ~(err <= bound)
        assert not bad.any(), (T, temp, int(bad.sum()), float(err.max()), np.argwhere(bad)[:4].tolist())
        # share of the fp32 term E used once the bf16 rounding is taken off (<= 1 by the assertion above)
        worst = max(worst, float(((err - 0.5 * _bf16_ulp(np.abs(r) + E)) / np.maximum(E, 2.0 ** -149)).max()))
        dl2 = _bwd(dy, ys, T, temp, temp_dev=torch.tensor([temp], dtype=torch.float32, device=DEV))
        assert torch.equal(_bits(dl2), _bits(dl)), (T, temp)
        for M in (1, 3):
            dlm = _bwd(dy[:M].clone(), ys[:M].clone(), T, temp)
            assert torch.equal(_bits(dlm), _bits(dl[:M])), (T, temp, M)
    REPORT[f"bwd_T{T}"] = dict(worst_err_beyond_rounding_over_fp32_bound=worst)
    print("gumbel bwd T", T, "worst (|dlogits - ref| - half ulp) / fp32 bound:", worst, flush=True)


# ------------------------------------------------------------------ MSE

def _mse_case(N, Cin, Cp, gs, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    img = torch.rand(N, Cin, generator=g, device=DEV) * 2 - 1
    out = (torch.randn(N, Cp, generator=g, device=DEV) * 0.7).to(torch.bfloat16)
    ws = torch.empty(dh.mse_workspace_bytes(), dtype=torch.uint8, device=DEV)
    dout = torch.full((N, Cp), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    loss = torch.full((1,), float("nan"), device=DEV)
    dh.mse_loss(img, out, dout, loss, N, Cin, Cp, gs, ws)
    torch.cuda.synchronize()
    assert bool((dout[:, Cin:] == 0).all()), "pad channels of dout must be exactly 0"
    lr, dr = ref.mse(img.cpu().numpy(), out[:, :Cin].float().cpu().numpy(), Cin, gs)
    # loss: per-thread grid-stride sums of ceil(N*Cp / 262144) terms, 6 + 2 levels within the block, a 1024-partial tree in
    # dmi_sum_f32 (10 levels), the difference, square and the scale 1/(N*Cin): all terms are >= 0, so
    # |error| <= (n_seq + 24) 2^-24 loss
    n_seq = -(-N * Cp // (1024 * 256))
    lerr = abs(float(loss) - lr)
    assert lerr <= (n_seq + 24) * 2.0 ** -24 * lr, (N, Cin, Cp, gs, float(loss), lr)
    # dout: (out - img) and 2 gs / (N*Cin) in fp32 (a few fp32 ulp), then rounded to bf16: within one bf16 ulp
    dd = dout[:, :Cin].double().cpu().numpy()
    err = np.abs(dd - dr[:, :Cin])
    bad = ~(err <= _bf16_ulp(dr[:, :Cin]) + 2.0 ** -126)
    assert not bad.any(), (N, Cin, Cp, gs, int(bad.sum()), float(err.max()))
    # without dout: the same loss, and nothing written
    keep = dout.clone()
    loss2 = torch.zeros(1, device=DEV)
    dh.mse_loss(img, out, None, loss2, N, Cin, Cp, gs, ws)
    torch.cuda.synchronize()
    assert torch.equal(loss2, loss) and torch.equal(_bits(dout), _bits(keep))
    return lerr / lr


@pytest.mark.parametrize("N,Cin,Cp", [(12345, 3, 8), (4099, 12, 64), (777, 48, 64), (128 * 256 * 256, 3, 64)])
@pytest.mark.parametrize("gs", [1.0, 0.125])
def test_mse_loss_and_gradient_vs_float64(N, Cin, Cp, gs):
    """(128 * 256 * 256, 3, 64): vae_coco's reconstruction at its batch of 128 (64 padded channels, as the engine calls it);
    gs = 1/8: the 1/world of an 8-GPU run folded into the gradient"""
    rel = _mse_case(N, Cin, Cp, gs, seed=N + Cin)
    REPORT[f"mse_N{N}_C{Cin}_{Cp}_gs{gs}"] = dict(loss_rel_err=rel)
    print("mse", N, Cin, Cp, gs, "loss rel err", rel, flush=True)


# ------------------------------------------------------------------ exact kernels

def test_pad_unpad_channels_bit_exact():
    for N, Cin, Cp in ((601, 3, 8), (600001, 3, 8), (1001, 12, 64), (257, 8, 8)):   # 600001 x 8 > 16384 blocks of 256: grid stride
        g = torch.Generator().manual_seed(N)
        x = torch.randn(N, Cin, generator=g) * 3
        bits = x.view(torch.int32)
        # round-to-nearest-even ties (low half exactly 0x8000 on an even and on an odd bf16 mantissa), just below / above a tie
        bits[0::7] = (bits[0::7] & ~0xFFFF) | 0x8000
        bits[1::7] = (bits[1::7] & ~0x1FFFF) | 0x18000
        bits[2::7] = (bits[2::7] & ~0xFFFF) | 0x7FFF
        bits[3::7] = (bits[3::7] & ~0xFFFF) | 0x8001
        x[4, 0], x[5, 0] = -0.0, 3.3e38
        out = torch.full((N, Cp), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        dh.pad_channels(x.to(DEV), out, N, Cin, Cp)
        want = torch.from_numpy(ref.pad_channels(x.to(torch.bfloat16).view(torch.int16).numpy(), Cp))
        assert torch.equal(_bits(out), want), (N, Cin, Cp)
        back = torch.full((N, Cin), float("nan"), device=DEV)
        dh.unpad_channels(out, back, N, Cin, Cp)
        want_f = torch.from_numpy(ref.unpad_channels(out.float().cpu().numpy(), Cin))
        assert torch.equal(back.cpu().view(torch.int32), want_f.view(torch.int32)), (N, Cin, Cp)


def test_add_f32_bit_exact():
    for n in (1000, 3 * 2 ** 20 + 77):       # > 4096 blocks of 256: the grid-stride loop runs
        g = torch.Generator().manual_seed(n)
        a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-3
        d = a.to(DEV)
        dh.add_f32(d, b.to(DEV), n)
        assert torch.equal(d.cpu().view(torch.int32), (a + b).view(torch.int32)), n
        d = a.to(DEV)
        dh.add_f32(d, b.to(DEV), n - 13)        # only the first n - 13
        want = a.clone()
        want[:n - 13] += b[:n - 13]
        assert torch.equal(d.cpu().view(torch.int32), want.view(torch.int32)), n


def test_pixel_interleave_bit_exact():
    for B, Ht, Wt, C in ((1, 1, 1, 8), (2, 5, 3, 24), (3, 16, 32, 128), (1, 64, 64, 512)):
        g = torch.Generator().manual_seed(C + Ht)
        x = torch.randint(-32768, 32767, (4, B, Ht, Wt, C), generator=g, dtype=torch.int16)
        out = torch.full((B, 2 * Ht, 2 * Wt, C), SENTINEL, dtype=torch.int16, device=DEV)
        dh.pixel_interleave(x.to(DEV).view(torch.bfloat16), out.view(torch.bfloat16), B, Ht, Wt, C)
        assert torch.equal(out.cpu(), torch.from_numpy(ref.pixel_interleave(x.numpy()))), (B, Ht, Wt, C)


def _rand_bf16(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, generator=g)).to(torch.bfloat16)


def test_weight_gather_bit_exact():
    rng = np.random.default_rng(5)
    cases = [(16, 37, 24, n, n * 24 + 40) for n in (1, 2, 3, 4, 9, 16)]
    cases += [(4, 13, 5, 4, 4 * 5 + 3), (9, 512, 512, 9, 9 * 512 + 64)]   # odd Bn; 2.4 M outputs > 4096 blocks: grid stride
    for K, A, Bn, nsel, ldo in cases:
        inp = _rand_bf16(K * A * Bn, K * A + nsel).view(K, A, Bn)
        idx = [int(i) for i in rng.integers(0, K, nsel)]
        out = torch.full((A, ldo), SENTINEL, dtype=torch.int16, device=DEV)
        dh.weight_gather(inp.to(DEV), out.view(torch.bfloat16), A, Bn, idx, ldo)
        want = torch.from_numpy(ref.weight_gather(inp.view(torch.int16).numpy(), idx, ldo))
        assert torch.equal(out.cpu(), want), (K, A, Bn, idx, ldo)


def _run_batch(in_base, out_len, items):
    table, blocks = ref.gather_table(items)
    out = torch.full((out_len,), SENTINEL, dtype=torch.int16, device=DEV)
    dh.weight_gather_batch(in_base.to(DEV).view(torch.bfloat16), out.view(torch.bfloat16), torch.from_numpy(table).to(DEV),
                           table.shape[0], blocks)
    want = ref.weight_gather_batch(in_base.view(torch.int16).numpy(), np.full(out_len, SENTINEL, np.int16), table)
    return out.cpu(), torch.from_numpy(want)


def test_weight_gather_batch_hand_built_tables():
    rng = np.random.default_rng(11)
    n_in = 1 << 21
    in_base = _rand_bf16(n_in, 1)

    def item(A, Bn, idx, ldo, out_off):
        K = max(idx) + 1
        return (int(rng.integers(0, n_in - K * A * Bn)), out_off, A, Bn, idx, ldo)

    shapes = [
        (3, 5, [2, 0], 12),                        # 36 elements: far less than one 2048-element block
        (64, 16, [0, 1, 2, 3], 64),                 # 4096 = 2 blocks: ends exactly on a block boundary
        (32, 32, [1], 64),                          # exactly one block
        (256, 128, list(range(9)), 1216),           # 152 blocks
        (17, 8, list(range(15, -1, -1)), 136),      # nsel = 16
        (1, 8, [4], 8),                             # one row
    ]
    shapes += [(int(rng.integers(1, 40)), 8 * int(rng.integers(1, 9)), [int(i) for i in rng.integers(0, 16, int(rng.integers(1, 17)))], 0)
               for _ in range(60)]                  # many items
    items, off = [], 0
    for A, Bn, idx, ldo in shapes:
        ldo = ldo or len(idx) * Bn + 8 * int(rng.integers(0, 3))
        off += int(rng.integers(0, 3)) * 64        # gaps between the items' outputs stay untouched
        items.append(item(A, Bn, idx, ldo, off))
        off += A * ldo
    for sel in (items[:1], items[:6], items, items[6:] + items[:6]):
        got, want = _run_batch(in_base, off + 256, sel)
        assert torch.equal(got, want), len(sel)


def test_weight_gather_batch_vae_coco_table():
    """the table DiscreteVAE builds for vae_coco (dgrad and output-parity gathers of every layer) against one weight_gather
    per item on the same bf16 master copy"""
    from src.vae_tf import DiscreteVAE
    p = json.load(open(os.path.join(ROOT, "configs", "vae_coco.json")))
    vae = DiscreteVAE(num_tokens=p["num_tokens"], dimensions=p["dataset"]["image_size"], convblocks=p["convblocks"], batch_size=1,
                      use_bf16=True)
    vae.init_params(seed=5)
    torch.cuda.synchronize()
    T = vae._refresh_tables
    table = T["ga"].cpu().numpy()
    items = [(int(r[0]), int(r[1]), int(r[2]), int(r[3]), [int(i) for i in r[7:7 + int(r[4])]], int(r[5])) for r in table]
    t2, blocks = ref.gather_table(items)
    assert np.array_equal(t2, table) and blocks == T["blocks"]
    assert len(items) > 20 and max(len(it[4]) for it in items) == 9
    for in_off, out_off, A, Bn, idx, ldo in items:
        K = max(idx) + 1
        one = torch.full((A, ldo), SENTINEL, dtype=torch.int16, device=DEV)
        dh.weight_gather(vae.pb[in_off:in_off + K * A * Bn], one.view(torch.bfloat16), A, Bn, idx, ldo)
        batch = vae.wcopies[out_off:out_off + A * ldo].view(torch.int16)
        assert torch.equal(one.view(-1), batch), (in_off, out_off, A, Bn, idx, ldo)
    del vae
    torch.cuda.empty_cache()


def test_discrete_vae_refuses_more_tokens_than_the_gumbel_kernel_handles():
    from src.vae_tf import DiscreteVAE
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="4096"):
        DiscreteVAE(num_tokens=8192, dimensions=32, convblocks=[[1, 64]], batch_size=1)
    assert torch.cuda.memory_allocated() == before       # refused before any allocation
    DiscreteVAE(num_tokens=4096, dimensions=32, convblocks=[[1, 64]], batch_size=1)


def test_zz_save_report():
    from parity import save_report
    save_report("vae_kernels.json", REPORT)
