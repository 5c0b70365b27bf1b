"""The tolerance-free specification of the GEMM family (CPU only): integer inputs, exact expected values, bit equality.

If A, B, bias and residual are small integers (times a power of two shared by all terms of an output), every product and every partial
sum of an output is an integer multiple of one granule below 2^24 granules: exactly representable in fp32 IN ANY ORDER.  The fp32
accumulator of any tiling, split or reduce order therefore equals the exact result, and a bf16 output must be RNE_bf16(exact): one
rounding, to nearest, ties to even, after all fp32 adds.  That pins dropped or duplicated k-terms, tile tails, the rounding mode, ties
and double rounding, bit for bit, with no other kernel of the library as the reference.

  generator   non-zero integers in +-1..7 as bf16 (a dropped or duplicated term changes every output it belongs to), optionally times
              2^-e, e in {0, 1, 2}, per row of A and per row of Bt (the terms of an output still share one scale); bias / residual
              integers in +-1..63, ReLU sources integers in -3..3 (zeros are masked), bias weights +-1..7, row scales from ROWSCALES
  guard       max(|A| @ |B|^T + |bias| + |residual|) * max|rowscale| / granule < 2^24, asserted for every case (guard()) on the
              cheap upper bound K max|A| max|B| of the first term
  expected    float64 torch matmul (exact here), the epilogue in float64, ONE float32 -> bfloat16 conversion on the CPU (RNE)
  epilogues   C = relu(acc + bias) + residual;  ReLU mask: C = acc where src > 0, +0 elsewhere;  row scale: C = acc * rowscale[m]
  TN          dW = X^T dY;  dbias = column sums of dY, or w^T dY with bias weights
  split-K     C = RNE((sum over slabs) * rowscale)
  check()     bit equality; its failure report (count, first bad (m, n), its tile and in-tile coordinates, got / expected, and whether
              got is the truncated, ties-away or twice-rounded value there) is the diagnosis -- nobody reruns a failing kernel for one.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

BIAS, RELU, RESIDUAL, RELU_MASK, OUT_F32, ROWSCALE = 1, 2, 4, 8, 16, 32
ROWSCALES = (-1.0, 0.5, 1.0, 2.0, 3.0)
LIMIT = float(2 ** 24)

# want: the expected tensor (bf16 or fp32);  exact: the float64 value before the final rounding;  twice: what an epilogue that rounds
# to bf16 BEFORE its adds / scale would store (None where there is nothing to add);  guard: the exactness figure (< 2^24)
Expected = namedtuple("Expected", "want exact twice guard")


# ------------------------------------------------------------------ generator

def ints(shape, seed, hi=7, zero=False):
    """integers in +-1..hi (zero=True: -hi..hi), float64"""
    g = torch.Generator().manual_seed(seed)
    if zero:
        return torch.randint(-hi, hi + 1, shape, generator=g).double()
    mag = torch.randint(1, hi + 1, shape, generator=g)
    sgn = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (mag * sgn).double()


def pow2_rows(rows, seed):
    """2^-e per row, e in {0, 1, 2}"""
    g = torch.Generator().manual_seed(seed)
    return torch.pow(2.0, -torch.randint(0, 3, (rows, 1), generator=g).double())


def rowscales(M, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(ROWSCALES)[torch.randint(0, len(ROWSCALES), (M,), generator=g)].float()


def bf(x):
    y = x.to(torch.bfloat16)
    assert torch.equal(y.double(), x.double()), "generator value is not a bf16 number"
    return y


def nt_inputs(M, N, K, seed=0, pow2=True):
    """operands of C[M, N] = A[M, K] . Bt[N, K]^T and every epilogue operand (bf16; rowscale fp32); `granule` = the smallest unit of
    any term of any output"""
    A, Bt = ints((M, K), 11 * seed + 1), ints((N, K), 11 * seed + 2)
    granule = 1.0
    if pow2:
        A, Bt = A * pow2_rows(M, 11 * seed + 3), Bt * pow2_rows(N, 11 * seed + 4)
        granule = 2.0 ** -4
    return dict(M=M, N=N, K=K, A=bf(A), Bt=bf(Bt), bias=bf(ints((N,), 11 * seed + 5, hi=63)), residual=bf(ints((M, N), 11 * seed + 6, hi=63)),
                relu_src=bf(ints((M, N), 11 * seed + 7, hi=3, zero=True)), rowscale=rowscales(M, 11 * seed + 8), granule=granule)


def tn_inputs(M, I, J, seed=0):
    """operands of dW[I, J] = X[M, I]^T . dY[M, J] and the bf16 bias weights [M]"""
    return dict(M=M, I=I, J=J, X=bf(ints((M, I), 13 * seed + 1)), dY=bf(ints((M, J), 13 * seed + 2)), w=bf(ints((M,), 13 * seed + 3)))


# ------------------------------------------------------------------ bf16 roundings of an fp32 value, on the bits

def _bits32(x):
    return x.float().contiguous().view(torch.int32)


def rne(x):
    """float32 -> bfloat16, to nearest, ties to even (the CPU conversion)"""
    return x.float().to(torch.bfloat16)


def truncated(x):
    """float32 -> bfloat16 toward zero"""
    return (_bits32(x) & -65536).view(torch.float32).to(torch.bfloat16)


def ties_away(x):
    """float32 -> bfloat16 to nearest, ties away from zero (sign-magnitude: add half an ulp to the magnitude, cut)"""
    return ((_bits32(x) + 0x8000) & -65536).view(torch.float32).to(torch.bfloat16)


def raw(t):
    t = t.contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def f32_exact(v64):
    v = v64.float()
    assert torch.equal(v.double(), v64), "the expected value is not an fp32 number: the exactness guard is wrong"
    return v


# ------------------------------------------------------------------ the specification

def guard(absacc_max, add_max=0.0, scale_max=1.0, granule=1.0):
    g = (absacc_max + add_max) * scale_max / granule
    assert g < LIMIT, f"exactness guard: {g:.4g} >= 2^24 -- the fp32 result would depend on the summation order"
    return g


def nt_guard(amax, flags, granule):
    """the guard of an NT case from `amax` >= max(|A| @ |Bt|^T): bias and residual are at most 63 each, a row scale at most 3 and
    its 0.5 halves the granule"""
    add = (63.0 if flags & BIAS else 0.0) + (63.0 if flags & RESIDUAL else 0.0)
    smax, gran = (max(abs(s) for s in ROWSCALES), granule / 2) if flags & ROWSCALE else (1.0, granule)
    return guard(amax, add, smax, gran)


def nt_acc(c):
    """(exact float64 product, an upper bound of max(|A| @ |Bt|^T): K times the largest magnitudes)"""
    A, Bt = c["A"].double(), c["Bt"].double()
    return A @ Bt.t(), float(A.abs().max()) * float(Bt.abs().max()) * c["K"]


def nt_epilogue(acc, c, flags, pre=lambda v: v):
    """the epilogue in float64 on `pre(acc)`; pre = identity: the specification"""
    v = pre(acc)
    if flags & BIAS:
        v = v + c["bias"].double()
    if flags & RELU:
        v = torch.relu(v)
    if flags & RESIDUAL:
        v = v + c["residual"].double()
    if flags & RELU_MASK:
        v = torch.where(c["relu_src"].double() > 0, v, torch.zeros_like(v))
    if flags & ROWSCALE:
        v = v * c["rowscale"].double()[:, None]
    return v


def nt_expected(c, flags, acc=None, amax=None):
    """Expected of dmi_gemm_nt(flags) -- also of the split-K form (flags 0 or ROWSCALE: the slabs sum to the same exact accumulator).
    acc / amax: a product computed elsewhere (the convolutions) and the bound of its sum of magnitudes"""
    if acc is None:
        acc, amax = nt_acc(c)
    g = nt_guard(amax, flags, c["granule"])
    exact = nt_epilogue(acc, c, flags)
    v32 = f32_exact(exact)
    if flags & OUT_F32:
        return Expected(v32, exact, None, g)
    twice = None
    if flags & (BIAS | RESIDUAL | ROWSCALE):
        twice = rne(nt_epilogue(acc, c, flags, pre=lambda v: rne(v).double()))
    return Expected(rne(v32), exact, twice, g)


def tn_expected(c):
    """(Expected of dW, of dbias = the column sums of dY, of dbias = w^T dY) of dmi_gemm_tn: fp32 outputs, compared as they are"""
    X, dY = c["X"].double(), c["dY"].double()
    g = guard(49.0 * c["M"])
    dW, db, dbw = X.t() @ dY, dY.sum(0), c["w"].double() @ dY
    return tuple(Expected(f32_exact(v), v, None, g) for v in (dW, db, dbw))


def conv_pad(taps, H, W, Ho, Wo, stride):
    """the zero padding (left, right, top, bottom) and kernel size under which F.conv2d walks a tap list, and each tap's kernel cell"""
    dys, dxs = [t[0] for t in taps], [t[1] for t in taps]
    y0, x0 = min(dys), min(dxs)
    kh, kw = max(dys) - y0 + 1, max(dxs) - x0 + 1
    top, left = -y0, -x0
    bottom = (Ho - 1) * stride + max(dys) - (H - 1)
    right = (Wo - 1) * stride + max(dxs) - (W - 1)
    return (left, right, top, bottom), (kh, kw), [(dy - y0, dx - x0) for dy, dx in taps]


def conv_weight(Wt, taps, C, cells, ksize):
    """Wt [N, ntaps * C] (tap-major) -> the float64 conv2d weight [N, C, kh, kw]"""
    N = Wt.shape[0]
    w = torch.zeros(N, C, *ksize, dtype=torch.float64)
    for t, (ky, kx) in enumerate(cells):
        w[:, :, ky, kx] = Wt[:, t * C:(t + 1) * C].double()
    return w


def conv_image(x, B, H, W, C, pad):
    """NHWC rows [B * H * W, C] -> padded float64 NCHW (negative padding crops)"""
    return F.pad(x.double().view(B, H, W, C).permute(0, 3, 1, 2), pad)


def conv_expected(x, B, H, W, C, Ho, Wo, stride, taps, Wt, c, flags):
    """Expected of dmi_conv_gemm_nt: float64 F.conv2d on the integer image and weights, then the epilogue of `c` (an nt_inputs dict with
    M = B * Ho * Wo rows)"""
    pad, ksize, cells = conv_pad(taps, H, W, Ho, Wo, stride)
    out = F.conv2d(conv_image(x, B, H, W, C, pad), conv_weight(Wt, taps, C, cells, ksize), stride=stride)
    assert out.shape[2:] == (Ho, Wo), out.shape
    acc = out.permute(0, 2, 3, 1).reshape(B * Ho * Wo, -1)
    return nt_expected(c, flags, acc=acc, amax=49.0 * len(taps) * C)


def conv_wgrad_expected(x, B, H, W, C, Ho, Wo, stride, taps, dY):
    """(Expected of dW [ntaps * C, N], Expected of dbias): the gradient of float64 F.conv2d with respect to its weight"""
    N = dY.shape[1]
    pad, ksize, cells = conv_pad(taps, H, W, Ho, Wo, stride)
    w = torch.zeros(N, C, *ksize, dtype=torch.float64, requires_grad=True)
    out = F.conv2d(conv_image(x, B, H, W, C, pad), w, stride=stride)
    out.backward(dY.double().view(B, Ho, Wo, N).permute(0, 3, 1, 2))
    dW = torch.stack([w.grad[:, :, ky, kx] for ky, kx in cells]).permute(0, 2, 1).reshape(len(taps) * C, N).contiguous()
    g = guard(49.0 * B * Ho * Wo)
    db = dY.double().sum(0)
    return Expected(f32_exact(dW), dW, None, g), Expected(f32_exact(db), db, None, g)


# ------------------------------------------------------------------ how much rounding a case exercises

def shares(e):
    """(share of outputs that are no bf16 number, share that are exact ties) of an Expected"""
    v = f32_exact(e.exact)
    low = _bits32(v) & 0xffff
    return float((low != 0).float().mean()), float((low == 0x8000).float().mean())


# ------------------------------------------------------------------ the check

def check(got, expected, what, tile=(128, 128)):
    """bit equality of `got` with the expected tensor (an Expected or a plain tensor); the failure message is the diagnosis"""
    e = expected if isinstance(expected, Expected) else Expected(expected, None, None, None)
    got = got.detach().cpu()
    want = e.want
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: got {tuple(got.shape)} {got.dtype}, expected {tuple(want.shape)} {want.dtype}"
    if torch.equal(raw(got), raw(want)):
        return
    bad = raw(got) != raw(want)
    g2, w2, b2 = (t.reshape(-1, t.shape[-1]) if t.dim() > 1 else t.reshape(1, -1) for t in (got, want, bad))
    m, n = (int(i) for i in b2.nonzero()[0])
    tm, tn = tile
    rows = b2.any(1).nonzero().flatten()
    cols = b2.any(0).nonzero().flatten()
    msg = (f"{what}: {int(bad.sum())}/{bad.numel()} outputs differ in their bits (rows {int(rows[0])}..{int(rows[-1])}, columns "
           f"{int(cols[0])}..{int(cols[-1])}); first at (m, n) = ({m}, {n}) = tile ({m // tm}, {n // tn}) + ({m % tm}, {n % tn}) of "
           f"{tm}x{tn}: got {float(g2[m, n])!r} (0x{int(raw(g2)[m, n]) & (0xffff if got.dtype == torch.bfloat16 else 0xffffffff):x}), "
           f"expected {float(w2[m, n])!r}")
    if e.exact is not None:
        x = e.exact.reshape(b2.shape)[m, n]
        msg += f", exact {float(x)!r}"
        if got.dtype == torch.bfloat16:
            x32 = x.float().reshape(1)
            kinds = [("the TRUNCATED value", truncated(x32)[0]), ("the TIES-AWAY value", ties_away(x32)[0])]
            if e.twice is not None:
                kinds.append(("the TWICE-ROUNDED value (bf16 before the adds / scale)", e.twice.reshape(b2.shape)[m, n]))
            hit = [k for k, v in kinds if int(raw(v.reshape(1))[0]) == int(raw(g2)[m, n])]
            msg += "; got is " + (" and ".join(hit) if hit else "none of truncated / ties-away / twice-rounded")
            ulp = float(torch.tensor(2.0) ** (torch.floor(torch.log2(x32.abs().clamp_min(1e-30))) - 7))
            msg += f"; error {(float(g2[m, n]) - float(x)) / ulp:+.3f} ulp"
        else:
            msg += f"; difference {float(g2[m, n]) - float(x):+.6g}"
    raise AssertionError(msg)


# ------------------------------------------------------------------ the cases of tests/test_gemm_exact_gpu.py
# Listed here so that tests/test_gemm_exact_ref.py holds every one of them to the guard and the tie shares on the CPU.  Each arm is
# forced with the option values the existing tests use for it, on shape classes they run; the smallest shapes with M and N tails, an
# odd and an even count of k-steps, more than one tile, and every epilogue of dmi_gemm_nt the arm is built for (NtTraits in gemm.hip:
# no fp32 output on the register-epilogue arms and the 256x128 tile; the skinny kernel has flags 0, 1, 3 and 5).

NT_ARMS = {"NT2": dict(nt4=0, nt8=0, nt8p=0, ntr=0), "NT4": dict(nt4=2), "NT8": dict(nt4=0, nt8=2), "NT8P": dict(nt4=0, nt8=0, nt8p=2),
           "NTR": dict(ntr=2), "SKINNY": dict(skinny=1)}
NT_TILE = {"NT2": (128, 128), "NT4": (256, 128), "NT8": (256, 256), "NT8P": (256, 256), "NTR": (160, 512), "SKINNY": (32, 16)}
_TILED = [(300, 256, 128, 0), (1000, 1160, 192, 1), (2100, 520, 384, 5), (515, 136, 64, 8), (700, 264, 128, 32), (130, 128, 448, 3)]
# (arm, extra options, M, N, K, flags)
NT_CASES = (
    [("NT2", {}, *s) for s in _TILED + [(300, 256, 128, 16)]]
    + [("NT4", {}, *s) for s in _TILED]
    + [("NT8", {}, *s) for s in _TILED + [(256, 256, 64, 16)]]
    # persistent: fewer tiles than blocks, K % 128 == 0, the register epilogues, several tiles per block with / without reserved CUs
    + [("NT8P", {}, *s) for s in [(300, 256, 128, 0), (1000, 1160, 256, 1), (2100, 520, 384, 3), (2100, 520, 384, 5), (515, 136, 128, 8),
                                  (700, 264, 128, 32)]]
    + [("NT8P", dict(reserve_cus=r), 6000, 5000, 128, 0) for r in (0, 16)]
    # full rows, N = 512: K / 32 = 4, 6, 8 (residues 1, 0, 2 mod 3), one whole tile, M tails, the residual in both register layouts
    + [("NTR", {}, *s) for s in [(160, 512, 128, 0), (333, 512, 192, 1), (333, 512, 192, 3), (1000, 512, 256, 8), (333, 512, 128, 32)]]
    + [("NTR", dict(res16=r), *s) for r in (1, 0) for s in [(333, 512, 256, 4), (1000, 512, 192, 5)]]
    + [("SKINNY", {}, *s) for s in [(32, 512, 512, 0), (3, 2048, 512, 3), (1, 16, 192, 5), (17, 48, 64, 1)]])

SPLITK_CASES = [({}, 300, 256, 1024, 2), ({}, 130, 128, 448, 3), (dict(nt4=0, nt8=2), 300, 256, 1024, 2)]     # (options, M, N, K, nsplit)

# fused entry points with an exact output: (options, M, N, K)
BITS_CASES = [(300, 256, 128), (2100, 576, 384)]
LN_CASES = [(160, 128, True), (1000, 256, True), (333, 160, False)]      # (M, K, with residual); N = 512
GELU_CASES = [(dict(skinny=0, ntr=0, nt8p=0, nt8=0, nt4=0), 333, 1000, 256), (dict(skinny=0, ntr=0, nt8p=2), 600, 512, 128), ({}, 7, 1024, 512)]
LABEL_CASES = [(300, 128, 1000), (77, 256, 777), (257, 64, 200)]         # (M, K, V)

# (arm, options, M, I, J): TN with / without the row-split tail launch, the 256x256 tile, the gang stream-K with another gang count
TN_CASES = (
    [("TN", dict(tn8=0, tn_tail=t), *s) for t in (1, 0) for s in [(72, 136, 200), (48, 128, 128), (544, 256, 384), (4096, 512, 256)]]
    + [("TAIL", dict(tn8=0, tn_tail=1), 200, 1024, 8320)]
    + [("TN8", dict(tn8=2), *s) for s in [(72, 136, 200), (544, 256, 384), (4096, 512, 256)]]
    + [("WIDE_SK", dict(reserve_cus=r), *s) for r in (0, 16) for s in [(33, 512, 40000), (200, 512, 33288)]])
TN_GROUPS = [(300, [(2048, 512, True)]), (1000, [(136, 200, True), (264, 72, True), (128, 128, False)]),
             (5000, [(512, 2048, True), (2048, 512, True), (512, 512, True), (512, 1536, False)])]

TAPS = {"3x3": [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)], "3x3rev": [(1 - ky, 1 - kx) for ky in range(3) for kx in range(3)],
        "4x4": [(ky - 1, kx - 1) for ky in range(4) for kx in range(4)], "par0": [(0, 0), (0, -1), (-1, 0), (-1, -1)],
        "par3": [(1, 1), (1, 0), (0, 1), (0, 0)]}
# (B, H, W, C, N, stride, kind, flags)
CONV_CASES = [(2, 12, 12, 64, 128, 1, "3x3", 0), (1, 16, 20, 128, 72, 1, "3x3rev", 4), (3, 8, 8, 64, 64, 1, "3x3", 8),
              (2, 16, 16, 64, 136, 2, "4x4", 1), (2, 9, 7, 64, 64, 1, "par0", 1), (1, 10, 6, 128, 64, 1, "par3", 0), (2, 6, 6, 192, 64, 1, "3x3", 3)]
# (B, H, W, C, N, stride, kind, with bias gradient)
WGRAD_CASES = [(2, 16, 16, 64, 128, 1, "3x3", True), (3, 8, 32, 128, 72, 1, "3x3", False), (2, 32, 32, 64, 64, 2, "4x4", True),
               (1, 64, 64, 192, 136, 1, "3x3", True)]
