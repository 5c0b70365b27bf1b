"""Every GEMM arm against the exact-integer specification of tests/gemm_exact_ref.py: bit equality, no tolerance.

The inputs are small integers (times a power of two per row), so the fp32 accumulator of any tiling, split or reduce order is the
exact result, a bf16 output must be RNE_bf16(exact) -- one rounding, to nearest-even, after all fp32 adds -- and an fp32 output the
exact value itself.  Each arm of NtKernel {SKINNY, NTR, NT8P, NT8, NT4, NT2} and TnKernel {TN, TN8, WIDE_SK, TAIL} (gemm_plan.h) is
forced with the option values the existing tests use for it, on their shape classes shrunk to the smallest that still has M and N
tails, odd and even k-step counts and more than one tile; the cases live in gemm_exact_ref (tests/test_gemm_exact_ref.py holds each
to the exactness guard and the tie shares on the CPU, and proves that check() rejects nine kinds of fault).

Per case: every output starts as NaN; lda > K (ldx > I, ldy > J, ldw > K), ldc > N and one NaN row behind every operand and output
wherever the entry point takes strides (the full-row fused form and the split-K form have fixed pitches); the pad columns and the
guard rows of the outputs must keep their NaN bits.  A NaN behind an input that reached a sum would poison the output.  Options go
through _options, which restores what get_option returned before, also when the case fails.  A failure's message is the diagnosis
(gemm_exact_ref.check): nobody reruns a failing kernel to find out.

Measured on an MI355X (every case prints its own EXACT line; shares of outputs that are no bf16 number / that are exact ties, range
over the arm's cases):

  family, arm                       cases   outputs compared                       rounded         ties            mismatches
  gemm_nt NT2  (128x128)                7   C bf16 (6), C fp32 (1)                 2.4 .. 38.3 %   2.4 .. 21.6 %   0
  gemm_nt NT4  (256x128)                6   C bf16                                 2.4 .. 38.3 %   2.4 .. 21.6 %   0
  gemm_nt NT8  (256x256)                7   C bf16 (6), C fp32 (1)                 2.4 .. 38.3 %   2.4 .. 21.6 %   0
  gemm_nt NT8P (persistent)             8   C bf16; reserve_cus 0 and 16           5.7 .. 38.3 %   5.2 .. 21.6 %   0
  gemm_nt NTR  (full rows)              9   C bf16; res16 1 and 0                  10.2 .. 30.5 %  7.8 .. 20.1 %   0
  gemm_nt SKINNY                        4   C bf16                                 17.3 .. 35.8 %  11.5 .. 22.2 %  0
  gemm_nt_splitk (NT2, NT8)             3   C bf16 without / with a row scale      32.8 .. 52.5 %  20.9 .. 22.5 %  0
  gemm_nt_relu_bits / _mask_bits        2   h bf16, masked product bf16            6.7 .. 17.5 %   6.1 .. 10.6 %   0
  gemm_nt_ln                            3   C bf16                                 25.6 .. 33.1 %  17.8 .. 20.4 %  0
  gemm_nt_gelu                          3   pre bf16                               23.7 .. 41.0 %  17.3 .. 22.5 %  0
  label_logit                           3   zl fp32                                -               -               0
  gemm_tn TN (tn_tail 1 and 0)          8   dW, dbias, weighted dbias fp32; twice  -               -               0
  gemm_tn TAIL                          1   the same                               -               -               0
  gemm_tn TN8                           3   the same                               -               -               0
  gemm_tn WIDE_SK (gang stream-K)       4   the same, cut stripes included         -               -               0
  gemm_tn_group, tn_wide 1 and 0        6   dW, dbias fp32; immediate = deferred   -               -               0
  conv_gemm_nt                          7   out bf16 vs float64 F.conv2d           14.5 .. 47.0 %  9.0 .. 22.8 %   0
  conv_wgrad_tn                         4   dW, dbias fp32 vs float64 F.conv2d     -               -               0

The whole file takes 7 s there, its slowest case 1.1 s ((6000, 5000, 128): 30 M outputs).  An experiment build of the library whose
float -> bf16 conversion cuts the low 16 bits (common.h: f2bf, pack2bf; nothing else changed) FAILED every case with a bf16 output
(53 of the 84 cases the file had then), each with check()'s diagnosis "got is the TRUNCATED value", and passed the 31 fp32 ones --
the fault the old tolerances accept (tests/test_gemm_exact_ref.py), on every NT arm.

An arm takes the epilogues it is built for (NtTraits): the residual on NT8P and ReLU, the mask and the row scale on NTR are forms
the dispatch can choose and no other test runs.  tests/test_gemm_exact_ref.py holds every case to the arm it is listed under by
asking gemm_plan.h itself.  Out of scope, with budget or parity tests of their own: the softmax
head's exponentials, the GELU values, the LayerNorm outputs, ln_gemm_nt and gemm_nt_lnbwd.
"""
import pytest
import torch

import gemm_exact_ref as gx
import dalle_hip as dh  # noqa: E402  (path set up by conftest)

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")

_CACHE = {}


class _options:
    """set the given options for a case; restore what get_option returned before, also when the case fails"""

    def __init__(self, *dicts):
        self.opts = {k: v for d in dicts for k, v in d.items()}

    def __enter__(self):
        self.saved = {k: dh.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            dh.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            dh.set_option(k, v)


def _nan(shape, dtype):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _padded(t, ld=None):
    """t [rows, cols] (or [n]) in the first rows / columns of a NaN-filled [rows + 1, ld] (or [n + 8]) device allocation"""
    if t.dim() == 1:
        full = _nan((t.numel() + 8,), t.dtype)
        full[:t.numel()] = t.to(DEV)
        return full
    rows, cols = t.shape
    full = _nan((rows + 1, ld or cols), t.dtype)
    full[:rows, :cols] = t.to(DEV)
    return full


def _exact(full, rows, cols, e, what, tile=(128, 128)):
    """the [rows, cols] block of `full` has the expected bits, and everything else in the allocation kept its NaN fill"""
    host = full.detach().cpu()
    body = host[:rows, :cols] if host.dim() == 2 else host[:cols]
    gx.check(body, e, what, tile=tile)
    bits = gx.raw(host)
    fill = int(gx.raw(torch.full((1,), NAN, dtype=host.dtype))[0])
    if host.dim() == 2:
        assert bool((bits[rows:] == fill).all()), f"{what}: rows behind the output were written"
        assert bool((bits[:rows, cols:] == fill).all()), f"{what}: pad columns of the output were written"
    else:
        assert bool((bits[cols:] == fill).all()), f"{what}: elements behind the output were written"
    if host.dtype == torch.bfloat16 and isinstance(e, gx.Expected):
        r, t = gx.shares(e)
        print(f"EXACT {what}: {e.want.numel()} outputs, rounded {100 * r:.1f} %, ties {100 * t:.1f} %, mismatches 0")
    else:
        print(f"EXACT {what}: {body.numel()} fp32 outputs, mismatches 0")


def _nt(M, N, K, flags, seed=None):
    key = ("nt", M, N, K, flags, seed)
    if key not in _CACHE:
        ikey = ("nti", M, N, K, seed)
        if ikey not in _CACHE:
            _CACHE[ikey] = gx.nt_inputs(M, N, K, seed=M + N + K if seed is None else seed)
        _CACHE[key] = (_CACHE[ikey], gx.nt_expected(_CACHE[ikey], flags))
    return _CACHE[key]


def _nt_operands(c, flags, ldc):
    K = c["K"]
    kw = dict(bias=c["bias"].to(DEV) if flags & gx.BIAS else None, residual=_padded(c["residual"], ldc) if flags & gx.RESIDUAL else None,
              relu_src=_padded(c["relu_src"], ldc) if flags & gx.RELU_MASK else None, rowscale=_padded(c["rowscale"]) if flags & gx.ROWSCALE else None)
    return _padded(c["A"], K + 64), K + 64, c["Bt"].to(DEV), kw


# ------------------------------------------------------------------ NT arms through dmi_gemm_nt

@pytest.mark.parametrize("arm,extra,M,N,K,flags", gx.NT_CASES)
def test_gemm_nt_arm_is_exact(arm, extra, M, N, K, flags):
    c, e = _nt(M, N, K, flags)
    ldc = N + 16
    A, lda, Bt, kw = _nt_operands(c, flags, ldc)
    C = _nan((M + 1, ldc), torch.float32 if flags & gx.OUT_F32 else torch.bfloat16)
    with _options(gx.NT_ARMS[arm], extra):
        dh.gemm_nt(A, lda, Bt, K, C, ldc, M, N, K, flags, **kw)
        torch.cuda.synchronize()
    _exact(C, M, N, e, f"gemm_nt {arm} {extra or ''} ({M}, {N}, {K}) flags {flags}", gx.NT_TILE[arm])


# ------------------------------------------------------------------ split-K

@pytest.mark.parametrize("opts,M,N,K,ns", gx.SPLITK_CASES)
def test_gemm_nt_splitk_is_exact(opts, M, N, K, ns):
    """fp32 slabs of an OUT_F32 launch, reduced to bf16 (ldc = N is part of the entry point): C = RNE(sum of the slabs [* rowscale])"""
    c, _ = _nt(M, N, K, 0)
    A, lda, Bt, _ = _nt_operands(c, 0, N)
    w = torch.empty(int(dh.gemm_nt_splitk_workspace_bytes(M, N, ns)) + 256, dtype=torch.uint8, device=DEV)
    for fl in (0, gx.ROWSCALE):
        e = _nt(M, N, K, fl)[1]
        C = _nan((M + 1, N), torch.bfloat16)
        with _options(opts):
            dh.gemm_nt_splitk(A, lda, Bt, K, C, M, N, K, ns, w, rowscale=_padded(c["rowscale"]) if fl else None)
            torch.cuda.synchronize()
        _exact(C, M, N, e, f"gemm_nt_splitk {opts or ''} ({M}, {N}, {K}) / {ns}" + (" row scale" if fl else ""))


# ------------------------------------------------------------------ NT entry points with an exact output

@pytest.mark.parametrize("M,N,K", gx.BITS_CASES)
def test_relu_bits_forms_are_exact(M, N, K):
    """h = RNE(relu(acc + bias)); the masked product of OTHER operands = RNE(acc2) where h > 0, +0 elsewhere"""
    c, e = _nt(M, N, K, gx.BIAS | gx.RELU)
    ldc = N + 16
    A, lda, Bt, _ = _nt_operands(c, 0, ldc)
    h = _nan((M + 1, ldc), torch.bfloat16)
    bits = torch.full((dh.relu_bits_bytes(M, N),), 0xAA, dtype=torch.uint8, device=DEV)
    dh.gemm_nt_relu_bits(A, lda, Bt, K, h, ldc, M, N, K, c["bias"].to(DEV), bits)
    torch.cuda.synchronize()
    _exact(h, M, N, e, f"gemm_nt_relu_bits ({M}, {N}, {K})", (256, 256))
    c2, e2 = _nt(M, N, K, 0, seed=7)
    keep = e.want.float() > 0
    assert 0.3 < float(keep.float().mean()) < 0.7
    exact2 = torch.where(keep, e2.exact, torch.zeros_like(e2.exact))
    A2, lda2, Bt2, _ = _nt_operands(c2, 0, ldc)
    g = _nan((M + 1, ldc), torch.bfloat16)
    dh.gemm_nt_mask_bits(A2, lda2, Bt2, K, g, ldc, M, N, K, bits)
    torch.cuda.synchronize()
    _exact(g, M, N, gx.Expected(gx.rne(gx.f32_exact(exact2)), exact2, None, e2.guard), f"gemm_nt_mask_bits ({M}, {N}, {K})", (256, 256))


@pytest.mark.parametrize("M,K,with_res", gx.LN_CASES)
def test_gemm_nt_ln_product_is_exact(M, K, with_res):
    """C of the fused product + LayerNorm (N = 512; C, the residual and Y have the pitch of a full row); Y keeps its own budget test"""
    N = 512
    flags = gx.BIAS | (gx.RESIDUAL if with_res else 0)
    c, e = _nt(M, N, K, flags)
    A, lda, Bt, kw = _nt_operands(c, flags, N)
    C, Y = _nan((M + 1, N), torch.bfloat16), _nan((M + 1, N), torch.bfloat16)
    mean, rstd = _nan((M + 8,), torch.float32), _nan((M + 8,), torch.float32)
    ones, zeros = torch.ones(N, dtype=torch.bfloat16, device=DEV), torch.zeros(N, dtype=torch.bfloat16, device=DEV)
    dh.gemm_nt_ln(A, lda, Bt, K, C, N, M, N, K, ones, zeros, Y, N, mean, rstd, bias=kw["bias"], residual=kw["residual"])
    torch.cuda.synchronize()
    _exact(C, M, N, e, f"gemm_nt_ln ({M}, {N}, {K}) flags {flags}", (160, 512))
    fill = int(gx.raw(torch.full((1,), NAN, dtype=torch.bfloat16))[0])
    assert bool((gx.raw(Y.cpu())[M:] == fill).all()) and bool(torch.isnan(mean[M:]).all()) and bool(torch.isnan(rstd[M:]).all())


@pytest.mark.parametrize("opts,M,N,K", gx.GELU_CASES)
def test_gemm_nt_gelu_preactivation_is_exact(opts, M, N, K):
    """pre = RNE(acc + bias); the GELU values have their own budget test"""
    c, e = _nt(M, N, K, gx.BIAS)
    ldc = N + 16
    A, lda, Bt, _ = _nt_operands(c, 0, ldc)
    C, pre = _nan((M + 1, ldc), torch.bfloat16), _nan((M + 1, ldc), torch.bfloat16)
    with _options(opts):
        dh.gemm_nt_gelu(A, lda, Bt, K, C, ldc, M, N, K, c["bias"].to(DEV), pre, ldc)
        torch.cuda.synchronize()
    _exact(pre, M, N, e, f"gemm_nt_gelu pre {opts or ''} ({M}, {N}, {K})")


@pytest.mark.parametrize("M,K,V", gx.LABEL_CASES)
def test_label_logit_is_exact(M, K, V):
    """zl[m] = X[m] . Wt[label[m]] + bias[label[m]] in fp32"""
    Vp = (V + 127) // 128 * 128
    c = gx.nt_inputs(M, Vp, K, seed=V)
    labels = torch.randint(0, V, (M,), generator=torch.Generator().manual_seed(V), dtype=torch.int32)
    lab = labels.long()
    exact = (c["A"].double() * c["Bt"].double()[lab]).sum(1) + c["bias"].double()[lab]
    e = gx.Expected(gx.f32_exact(exact), exact, None, gx.nt_guard(49.0 * K, gx.BIAS, c["granule"]))
    zl = _nan((M + 8,), torch.float32)
    flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    dh.label_logit(_padded(c["A"], K + 8), K + 8, _padded(c["Bt"], K + 8), K + 8, c["bias"].to(DEV), labels.to(DEV), zl, flag, M, K, V)
    torch.cuda.synchronize()
    _exact(zl, 1, M, e, f"label_logit ({M}, {K}, {V})")
    assert int(flag.item()) == 0


# ------------------------------------------------------------------ TN arms through dmi_gemm_tn

def _tn(M, I, J):
    key = ("tn", M, I, J)
    if key not in _CACHE:
        c = gx.tn_inputs(M, I, J, seed=M + I + J)
        eW, eb, ebw = gx.tn_expected(c)
        _CACHE[key] = (c, (eW, eb), ebw if M % 2 == 0 else None)     # (bias weights travel as dwords: an even M)
    return _CACHE[key]


def _ws(M, I, J):
    return torch.empty(int(dh.gemm_tn_workspace_bytes(M, I, J)) + 256, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("arm,opts,M,I,J", gx.TN_CASES)
def test_gemm_tn_arm_is_exact(arm, opts, M, I, J):
    """dW and dbias (column sums; with bias weights where M is even) exact on every plan: unsplit, split with a slab reduce, the
    row-split tail launch, the 256x256 tile, the gang stream-K whose cut stripes are two-addend atomic sums; run twice"""
    c, (eW, eb), ebw = _tn(M, I, J)
    X, dY, w = _padded(c["X"], I + 8), _padded(c["dY"], J + 8), _padded(c["w"])
    ws = _ws(M, I, J)
    with _options(opts):
        for rep in range(2):
            weighted = rep == 1 and ebw is not None
            dW, db = _nan((I + 1, J), torch.float32), _nan((J + 8,), torch.float32)
            dh.gemm_tn(X, I + 8, dY, J + 8, dW, M, I, J, ws, dbias=db, bias_weights=w if weighted else None)
            torch.cuda.synchronize()
            what = f"gemm_tn {arm} {opts} ({M}, {I}, {J}) run {rep}"
            _exact(dW, I, J, eW, what + " dW")
            _exact(db, 1, J, ebw if weighted else eb, what + (" weighted dbias" if weighted else " dbias"))


# ------------------------------------------------------------------ TN, grouped and deferred

@pytest.mark.parametrize("wide", [1, 0])
@pytest.mark.parametrize("M,shapes", gx.TN_GROUPS)
def test_gemm_tn_group_is_exact(M, shapes, wide):
    """one problem, the ragged three, the four gradients of a block (128 x 256 tiles under tn_wide 1): every dW and dbias exact, and
    the deferred reduces give the same exact bits"""
    probs, exp = [], []
    for I, J, with_bias in shapes:
        c, (eW, eb), _ = _tn(M, I, J)
        probs.append(dict(X=_padded(c["X"], I + 8), ldx=I + 8, dY=_padded(c["dY"], J + 8), ldy=J + 8, I=I, J=J, ws=_ws(M, I, J)))
        exp.append((eW, eb if with_bias else None))
    with _options(dict(tn_wide=wide)):
        assert (dh.gemm_tn_group_plan([(I, J) for I, J, _ in shapes], M) > 0) == (wide == 1 and len(shapes) == 4)
        for mode in ("immediate", "deferred"):
            for q, (eW, eb) in zip(probs, exp):
                q["dW"] = _nan((q["I"] + 1, q["J"]), torch.float32)
                if eb is not None:
                    q["dbias"] = _nan((q["J"] + 8,), torch.float32)
            dfr = dh.DeferredReduces() if mode == "deferred" else None
            dh.gemm_tn_group(probs, M, deferred=dfr)
            if dfr is not None:
                dfr.run()
            torch.cuda.synchronize()
            for q, (eW, eb) in zip(probs, exp):
                what = f"gemm_tn_group tn_wide {wide} {mode} M {M} ({q['I']}, {q['J']})"
                _exact(q["dW"], q["I"], q["J"], eW, what + " dW")
                if eb is not None:
                    _exact(q["dbias"], 1, q["J"], eb, what + " dbias")


# ------------------------------------------------------------------ convolutions against float64 F.conv2d

@pytest.mark.parametrize("B,H,W,C,N,stride,kind,flags", gx.CONV_CASES)
def test_conv_gemm_nt_is_exact(B, H, W, C, N, stride, kind, flags):
    taps = gx.TAPS[kind]
    Ho, Wo = H // stride, W // stride
    K, M = len(taps) * C, B * Ho * Wo
    x = gx.bf(gx.ints((B * H * W, C), seed=3 * K + 1))
    c = gx.nt_inputs(M, N, K, seed=K + N, pow2=False)
    e = gx.conv_expected(x, B, H, W, C, Ho, Wo, stride, taps, c["Bt"], c, flags)
    ldc = N + 8
    kw = dict(bias=c["bias"].to(DEV) if flags & gx.BIAS else None, residual=_padded(c["residual"], ldc) if flags & gx.RESIDUAL else None,
              relu_src=_padded(c["relu_src"], ldc) if flags & gx.RELU_MASK else None)
    out = _nan((M + 1, ldc), torch.bfloat16)
    dh.conv_gemm_nt(_padded(x), B, H, W, C, Ho, Wo, stride, taps, _padded(c["Bt"], K + 8), K + 8, out, ldc, N, flags, **kw)
    torch.cuda.synchronize()
    _exact(out, M, N, e, f"conv_gemm_nt {kind} ({B}, {H}, {W}, {C}) -> {N} flags {flags}")


@pytest.mark.parametrize("B,H,W,C,N,stride,kind,bias", gx.WGRAD_CASES)
def test_conv_wgrad_tn_is_exact(B, H, W, C, N, stride, kind, bias):
    taps = gx.TAPS[kind]
    Ho, Wo = H // stride, W // stride
    K, M = len(taps) * C, B * Ho * Wo
    x = gx.bf(gx.ints((B * H * W, C), seed=3 * K + 2))
    dY = gx.bf(gx.ints((M, N), seed=3 * K + 3))
    eW, eb = gx.conv_wgrad_expected(x, B, H, W, C, Ho, Wo, stride, taps, dY)
    dW, db = _nan((K + 1, N), torch.float32), _nan((N + 8,), torch.float32)
    ws = torch.empty(dh.conv_wgrad_tn_workspace_bytes(M, K, N) + 256, dtype=torch.uint8, device=DEV)
    dh.conv_wgrad_tn(_padded(x), B, H, W, C, Ho, Wo, stride, taps, _padded(dY, N + 8), N + 8, N, dW, ws, dbias=db if bias else None)
    torch.cuda.synchronize()
    what = f"conv_wgrad_tn {kind} ({B}, {H}, {W}, {C}) -> {N}"
    _exact(dW, K, N, eW, what + " dW")
    if bias:
        _exact(db, 1, N, eb, what + " dbias")
