"""The exact-integer GEMM specification of tests/gemm_exact_ref.py, checked on the CPU: the exactness guard holds for every case of
tests/test_gemm_exact_gpu.py, every bf16 family really exercises rounding and ties, the expected values do not depend on the
summation order, check() has teeth -- nine float32 emulations of kernel faults are each rejected, with the right diagnosis -- and the
tolerance the 128x128 kernel was held to before accepts the first of them (the gap these tests close).  The convolution references
(float64 F.conv2d) are held to an independent tap-by-tap gather."""
import math
import os
import shutil
import subprocess

import pytest
import torch

import gemm_exact_ref as gx

HERE = os.path.dirname(os.path.abspath(__file__))
_CACHE = {}


def _nt(M, N, K, flags):
    key = (M, N, K, flags)
    if key not in _CACHE:
        c = gx.nt_inputs(M, N, K, seed=M + N + K)
        _CACHE[key] = (c, gx.nt_expected(c, flags))
    return _CACHE[key]


def _rejected(got, e, what, tile=(128, 128)):
    with pytest.raises(AssertionError) as info:
        gx.check(got, e, what, tile=tile)
    return str(info.value)


# ------------------------------------------------------------------ the guard and the shares of rounded / tied outputs

def test_guard_holds_for_every_gpu_case():
    """from the cases' sizes alone (magnitudes <= 7, bias / residual <= 63, row scales <= 3, granule 2^-4 (halved by a row scale of
    0.5)): every fp32 partial sum of every case is exact, so its result is order-independent"""
    worst = 0.0
    for _, _, M, N, K, flags in gx.NT_CASES:
        worst = max(worst, gx.nt_guard(49.0 * K, flags, 2.0 ** -4))
    for _, M, N, K, ns in gx.SPLITK_CASES:
        worst = max(worst, gx.nt_guard(49.0 * K, gx.ROWSCALE, 2.0 ** -4))
    for M, N, K in gx.BITS_CASES:
        worst = max(worst, gx.nt_guard(49.0 * K, gx.BIAS | gx.RELU, 2.0 ** -4))
    for M, K, _ in gx.LN_CASES:
        worst = max(worst, gx.nt_guard(49.0 * K, gx.BIAS | gx.RESIDUAL, 2.0 ** -4))
    for _, M, N, K in gx.GELU_CASES:
        worst = max(worst, gx.nt_guard(49.0 * K, gx.BIAS, 2.0 ** -4))
    for M, K, V in gx.LABEL_CASES:
        worst = max(worst, gx.nt_guard(49.0 * K, gx.BIAS, 2.0 ** -4))
    for _, _, M, I, J in gx.TN_CASES:
        worst = max(worst, gx.guard(49.0 * M))
    for M, shapes in gx.TN_GROUPS:
        worst = max(worst, gx.guard(49.0 * M))
    for B, H, W, C, N, stride, kind, flags in gx.CONV_CASES:
        worst = max(worst, gx.nt_guard(49.0 * len(gx.TAPS[kind]) * C, flags, 1.0))
    for B, H, W, C, N, stride, kind, _ in gx.WGRAD_CASES:
        worst = max(worst, gx.guard(49.0 * B * (H // stride) * (W // stride)))
    print(f"GUARD worst case {worst:.4g} of {gx.LIMIT:.4g}")
    assert worst < gx.LIMIT
    with pytest.raises(AssertionError):      # ... and the guard itself refuses a case that is not exact: K = 2^19 at magnitude 49
        gx.nt_guard(49.0 * 2 ** 19, 0, 1.0)


def _families():
    """family -> [(label, Expected)] of every bf16 output the GPU file compares"""
    fam = {}
    for arm, _, M, N, K, flags in gx.NT_CASES:
        if not flags & gx.OUT_F32:
            fam.setdefault(arm, []).append(((M, N, K, flags), _nt(M, N, K, flags)[1]))
    for _, M, N, K, ns in gx.SPLITK_CASES:
        for fl in (0, gx.ROWSCALE):
            fam.setdefault("split-K", []).append(((M, N, K, fl), _nt(M, N, K, fl)[1]))
    for M, N, K in gx.BITS_CASES:
        fam.setdefault("relu_bits", []).append(((M, N, K), _nt(M, N, K, gx.BIAS | gx.RELU)[1]))
    for M, K, res in gx.LN_CASES:
        fl = gx.BIAS | (gx.RESIDUAL if res else 0)
        fam.setdefault("gemm_nt_ln", []).append(((M, 512, K), _nt(M, 512, K, fl)[1]))
    for _, M, N, K in gx.GELU_CASES:
        fam.setdefault("gelu pre", []).append(((M, N, K), _nt(M, N, K, gx.BIAS)[1]))
    for B, H, W, C, N, stride, kind, flags in gx.CONV_CASES:
        Ho, Wo = H // stride, W // stride
        K = len(gx.TAPS[kind]) * C
        c = gx.nt_inputs(B * Ho * Wo, N, K, seed=K + N, pow2=False)
        x = gx.bf(gx.ints((B * H * W, C), seed=3 * K + 1))
        fam.setdefault("conv", []).append(((B, H, W, C, N, kind), gx.conv_expected(x, B, H, W, C, Ho, Wo, stride, gx.TAPS[kind], c["Bt"], c, flags)))
    return fam


def test_every_bf16_family_exercises_rounding_and_ties():
    """every bf16 case with at least 10 000 outputs has at least 1 % exact ties (and as many outputs again that need rounding at all);
    smaller cases meet the condition over their family.  -s prints the shares of every case."""
    for name, cases in _families().items():
        tot = ties = 0
        for label, e in cases:
            r, t = gx.shares(e)
            n = e.want.numel()
            print(f"SHARES {name:10s} {str(label):32s} outputs {n:9d}  rounded {100 * r:5.1f} %  ties {100 * t:5.1f} %")
            tot += n
            ties += t * n
            assert r >= t
            if n >= 10000:
                assert t >= 0.01, (name, label, r, t)
        assert ties / tot >= 0.01, (name, ties / tot)


def test_shares_grow_with_k():
    """the sums are about 20 sqrt(K) wide and integers above 256 are no bf16 numbers: the longer K, the more outputs round"""
    got = []
    for M, N, K in [(300, 256, 64), (300, 256, 128), (2100, 520, 384), (1024, 512, 2048)]:
        c = gx.nt_inputs(M, N, K, seed=1, pow2=False)
        r, t = gx.shares(gx.nt_expected(c, 0))
        print(f"SHARES plain ({M}, {N}, {K}): rounded {100 * r:.1f} %, ties {100 * t:.1f} %")
        got.append((r, t))
    assert all(a[0] < b[0] for a, b in zip(got, got[1:]))
    assert got[0][1] > 0.03 and got[-1][0] > 0.5 and got[-1][1] > 0.15


# ------------------------------------------------------------------ every case runs on the arm it is listed under

def test_every_arm_of_the_dispatch_plan_is_reached(tmp_path):
    """tests/host/gemm_exact_arms.cpp asks gemm_plan.h (host-only C++) for the kernel of each case under the case's options on the
    256 CUs of an MI355X, with the leading dimensions the GPU file passes: the arm the case is listed under, and the lists cover all
    of NtKernel and TnKernel"""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "gemm_exact_arms")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(HERE, "host", "gemm_exact_arms.cpp"), "-o", exe], check=True)
    opt = lambda *ds: " ".join(f"{k} {v}" for d in ds for k, v in d.items())
    lines, want = [], []
    for arm, extra, M, N, K, flags in gx.NT_CASES:
        lines.append(f"NT {M} {N} {K} {K + 64} {K} {K} 1 {flags} 256 {opt(gx.NT_ARMS[arm], extra)}")
        want.append(arm)
    for opts, M, N, K, ns in gx.SPLITK_CASES:
        kps = ((K + ns - 1) // ns + 63) // 64 * 64
        lines.append(f"NT {M} {N} {K} {K + 64} {K} {kps} {(K + kps - 1) // kps} {gx.OUT_F32} 256 {opt(opts)}")
        want.append("NT8" if opts else "NT2")
    for arm, opts, M, I, J in gx.TN_CASES:
        lines.append(f"TN {M} {I} {J} 256 {opt(opts)}")
        want.append(arm)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.split()
    assert got == want, [(ln, g, w) for ln, g, w in zip(lines, got, want) if g != w]
    assert set(got) == {"SKINNY", "NTR", "NT8P", "NT8", "NT4", "NT2", "TN", "TN8", "WIDE_SK", "TAIL"}


# ------------------------------------------------------------------ the expected values do not depend on the order

@pytest.mark.parametrize("M,N,K,flags", [(300, 256, 128, 0), (130, 128, 448, 3), (515, 136, 64, 8), (700, 264, 128, 32), (300, 256, 128, 5),
                                         (300, 256, 128, 16)])
def test_float32_in_any_order_meets_the_specification(M, N, K, flags):
    """a float32 emulation of a correct kernel -- k in 32-wide chunks, last chunk first, two interleaved partial accumulators, the
    epilogue in float32, one rounding -- passes check() bit for bit"""
    c, e = _nt(M, N, K, flags)
    A, Bt = c["A"].float(), c["Bt"].float()
    acc = [torch.zeros(M, N), torch.zeros(M, N)]
    for i, k0 in enumerate(reversed(range(0, K, 32))):
        acc[i & 1] = acc[i & 1] + A[:, k0:k0 + 32] @ Bt[:, k0:k0 + 32].t()
    v = gx.nt_epilogue((acc[0] + acc[1]).double(), c, flags).float()
    gx.check(v if flags & gx.OUT_F32 else gx.rne(v), e, "float32 emulation")


# ------------------------------------------------------------------ faults that check() must reject

M0, N0, K0 = 300, 256, 128


def _acc32(c, k1=None):
    return (c["A"].float()[:, :k1] @ c["Bt"].float()[:, :k1].t())


def test_fault_truncation_is_rejected_and_the_old_tolerance_accepts_it():
    """1. an epilogue that cuts the low 16 bits instead of rounding to nearest-even: at most 1 ulp = 2^-7 relative -- inside the rtol
    1.6e-2 + atol 2e-2 sqrt(K / 64) the 128x128 kernel was held to against fp32 torch (tests/test_kernels_gpu.py: close)"""
    c, e = _nt(M0, N0, K0, 0)
    got = gx.truncated(_acc32(c))
    msg = _rejected(got, e, "truncation")
    assert "the TRUNCATED value" in msg and "TIES-AWAY" not in msg, msg
    ref = _acc32(c)
    err = (got.float() - ref).abs()
    assert float(err.max()) > 0
    assert not bool((err > 2e-2 * math.sqrt(K0 / 64) + 1.6e-2 * ref.abs()).any()), "the old tolerance was expected to accept truncation"
    assert float((err / ref.abs().clamp_min(1e-30)).max()) < 2.0 ** -7


def test_fault_ties_away_from_zero_is_rejected():
    """2. round-half-away: differs from RNE on the ties whose kept mantissa is even"""
    c, e = _nt(M0, N0, K0, 0)
    msg = _rejected(gx.ties_away(_acc32(c)), e, "ties away")
    assert "the TIES-AWAY value" in msg and "TRUNCATED" not in msg, msg


@pytest.mark.parametrize("flags,name", [(gx.BIAS, "bias"), (gx.RESIDUAL, "residual"), (gx.BIAS | gx.RESIDUAL, "bias + residual"),
                                        (gx.ROWSCALE, "row scale")])
def test_fault_add_after_the_rounding_is_rejected(flags, name):
    """3. / 4. bias, residual (or the row scale) applied to the bf16-rounded accumulator: two roundings"""
    c, e = _nt(M0, N0, K0, flags)
    got = gx.rne(gx.nt_epilogue(gx.rne(_acc32(c)).double(), c, flags).float())
    msg = _rejected(got, e, name + " after the rounding")
    assert "TWICE-ROUNDED" in msg, msg


@pytest.mark.parametrize("M,N,K,ns", [(300, 256, 1024, 2), (130, 128, 448, 3)])
def test_fault_splitk_slabs_in_bf16_and_slab_counted_twice_are_rejected(M, N, K, ns):
    """5. split-K partials kept as bf16 before the reduce; 9. one slab added twice -- in the bf16 result and in an fp32 one"""
    c, e = _nt(M, N, K, 0)
    kps = ((K + ns - 1) // ns + 63) // 64 * 64
    slabs = [c["A"].float()[:, k0:k0 + kps] @ c["Bt"].float()[:, k0:k0 + kps].t() for k0 in range(0, K, kps)]
    gx.check(gx.rne(sum(slabs)), e, "fp32 slabs")          # (the correct reduce passes)
    _rejected(gx.rne(sum(gx.rne(s).float() for s in slabs)), e, "bf16 slabs")
    _rejected(gx.rne(sum(slabs) + slabs[0]), e, "slab 0 twice")
    e32 = gx.nt_expected(c, gx.OUT_F32)
    msg = _rejected(sum(slabs) + slabs[-1], e32, "last slab twice, fp32")
    bad = int(msg.split(": ")[1].split("/")[0])            # every output whose slab sum is not zero changes
    assert bad == int((slabs[-1] != 0).sum()) and bad > 0.99 * M * N, msg


def test_fault_dropped_k_term_and_skipped_k_step_are_rejected():
    """6. one k-term dropped in one tile: every fp32 output of that tile changes (the operands have no zeros), and the report names
    the tile; 7. the last k-step skipped"""
    c, e = _nt(M0, N0, K0, 0)
    e32 = gx.nt_expected(c, gx.OUT_F32)
    acc = _acc32(c)
    drop = acc.clone()
    drop[128:256, 128:256] -= c["A"].float()[128:256, 77:78] @ c["Bt"].float()[128:256, 77:78].t()
    msg = _rejected(drop, e32, "dropped k-term, fp32")
    assert f"{128 * 128}/{M0 * N0}" in msg and "tile (1, 1) + (0, 0)" in msg and "rows 128..255, columns 128..255" in msg, msg
    msg = _rejected(gx.rne(drop), e, "dropped k-term, bf16")
    assert "tile (1, 1)" in msg, msg
    _rejected(gx.rne(_acc32(c, K0 - 64)), e, "last k-step skipped")
    _rejected(_acc32(c, K0 - 64), e32, "last k-step skipped, fp32")


def test_fault_unstored_tail_row_is_rejected():
    """8. the last row of the M tail left as the output's NaN fill"""
    c, e = _nt(M0, N0, K0, 0)
    got = e.want.clone()
    got[M0 - 1] = float("nan")
    msg = _rejected(got, e, "tail row")
    assert f"first at (m, n) = ({M0 - 1}, 0) = tile (2, 0) + ({M0 - 1 - 256}, 0)" in msg, msg
    gx.check(e.want.clone(), e, "the expected value itself")
    neg0 = e.want.clone()                                   # bits, not values: -0 for +0 is a difference
    z = (neg0 == 0).nonzero()
    if len(z):
        neg0[tuple(z[0])] = -0.0
        _rejected(neg0, e, "-0 for +0")


def test_fault_tn_dropped_rows_and_unweighted_bias_are_rejected():
    """the same for the fp32 weight gradient: the last row missing (every output changes: no operand is zero), a 32-row step
    missing, the bias weights ignored"""
    c = gx.tn_inputs(200, 136, 72, seed=1)
    eW, _, eb = gx.tn_expected(c)
    X, dY = c["X"].float(), c["dY"].float()
    gx.check(X.t() @ dY, eW, "dW")
    gx.check(c["w"].float() @ dY, eb, "dbias")
    msg = _rejected(X[:-1].t() @ dY[:-1], eW, "dW without the last row")
    assert f"{136 * 72}/{136 * 72}" in msg, msg
    _rejected(X[:-32].t() @ dY[:-32], eW, "dW without the last step")
    _rejected(dY.sum(0), eb, "unweighted dbias")


# ------------------------------------------------------------------ the convolution references against a tap-by-tap gather

def _im2col64(x, B, H, W, C, Ho, Wo, stride, taps):
    img = x.double().view(B, H, W, C)
    col = torch.zeros(B, Ho, Wo, len(taps), C, dtype=torch.float64)
    for t, (dy, dx) in enumerate(taps):
        for oy in range(Ho):
            iy = oy * stride + dy
            if not 0 <= iy < H:
                continue
            for ox in range(Wo):
                ix = ox * stride + dx
                if 0 <= ix < W:
                    col[:, oy, ox, t] = img[:, iy, ix]
    return col.view(B * Ho * Wo, len(taps) * C)


@pytest.mark.parametrize("B,H,W,C,N,stride,kind", [(2, 5, 6, 8, 16, 1, "3x3"), (1, 4, 6, 8, 8, 1, "3x3rev"), (2, 8, 4, 8, 8, 2, "4x4"),
                                                   (2, 9, 7, 8, 8, 1, "par0"), (1, 10, 6, 8, 8, 1, "par3")])
def test_conv_references_equal_the_gathered_product(B, H, W, C, N, stride, kind):
    taps = gx.TAPS[kind]
    Ho, Wo = H // stride, W // stride
    K, M = len(taps) * C, B * Ho * Wo
    x = gx.bf(gx.ints((B * H * W, C), seed=5))
    c = gx.nt_inputs(M, N, K, seed=6, pow2=False)
    col = _im2col64(x, B, H, W, C, Ho, Wo, stride, taps)
    e = gx.conv_expected(x, B, H, W, C, Ho, Wo, stride, taps, c["Bt"], c, gx.BIAS | gx.RESIDUAL)
    want = gx.nt_epilogue(col @ c["Bt"].double().t(), c, gx.BIAS | gx.RESIDUAL)
    assert torch.equal(e.exact, want)
    dY = gx.bf(gx.ints((M, N), seed=7))
    eW, eb = gx.conv_wgrad_expected(x, B, H, W, C, Ho, Wo, stride, taps, dY)
    assert torch.equal(eW.exact, col.t() @ dY.double()) and torch.equal(eb.exact, dY.double().sum(0))
