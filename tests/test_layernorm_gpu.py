"""The six LayerNorm kernels against the float64 specification under the error budget of tests/layernorm_ref.py: y and dx by the row
metric against the bf16 emulation (MARGIN_MAX / MARGIN_MED, imported), mean / rstd and dgamma / dbeta by derived bounds, constant rows
element by element.  Inputs are the families of layernorm_ref (offsets, near-constant rows, tiny and huge scales, rows of every scale
in one launch), at widths with partly filled chunk groups, a single chunk, all four NC instances, ragged row blocks, two eps.

Every fused kernel is judged on what it stored: dropout_add_ln on its x_out, gemm_nt_ln on its C, so only the LayerNorm is judged;
gemm_nt_lnbwd against the float64 product for dx (the emulation rounds dy to bf16, the kernel may or may not) and, for dgamma / dbeta,
against the bf16 product the same main loop stores through gemm_nt_ln (dy's bf16 rounding is part of the kernel's definition and
2^-9 relative, far above the fp32 summation bound of the gradients; that stored product is itself held to half a bf16 ulp + the fp32
accumulation bound of the float64 one).  The two fused full-row products take K = 160, five k-steps of 32.

Measured on an MI355X (every case prints its own RATIO line): worst ratio over the kernel's cases of the kernel's row error over the
emulation's (max, median) and of each statistic's / gradient's error over its derived bound.

  kernel          cases          y, dx or C / emulation (max, median)   const rows   mean     rstd     dgamma    dbeta
  layernorm_fwd   16             1.0000  1.0000                         0            0.0154   0.127    -         -
  layernorm_bwd   40 (720 runs)  1.0000  1.0000                         -            -        -        0.0674    0.0105
  dropout_add_ln  4              1.0000  1.0000                         0            0.0095   0.0447   -         -
  gemm_nt_ln      2              1.0000  1.0000                         0            0.0126   0.0801   -         -
  gemm_nt_lnbwd   4              1.0000  1.0000                         -            -        -        0.00404   0.000703
  ln_gemm_nt      6              1.0000  1.0000                         0 (ulps)     -        -        -         -

The kernels round the same fp32 values to bf16 as the emulation does -- their statistics differ from torch's in the last bits (the
mean / rstd columns: at most an eighth of the derived bounds), which hardly ever flips a bf16 rounding -- so the row
ratios sit at 1 and the margins in force are the imported ones.  On constant rows every kernel
returns beta (ln_gemm_nt: bf16(beta . Bt^T)) exactly.  tests/test_layernorm_ref.py proves that the budget rejects the seeded faults.
"""
import pytest
import torch

import dropout_ref
import layernorm_ref as lr
import dalle_hip as dh  # noqa: E402  (path set up by conftest)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = 37           # not a multiple of the 4 rows of a forward block
G = 8               # sentinel rows behind every output
N_FULL = 512        # the width of the full-row products

_CACHE = {}


def _stacked(d, eps):
    """37 rows of every family, one after the other, drawn once per d; the forward's inputs dict per (d, eps)"""
    if ("x", d) not in _CACHE:
        _CACHE[("x", d)] = lr.stacked(lr.FAMILIES, ROWS, d, seed=10 * d) + lr.params(d, seed=d)
    x, groups, gamma, beta = _CACHE[("x", d)]
    if ("f", d, eps) not in _CACHE:
        _CACHE[("f", d, eps)] = lr.make_inputs_fwd(x, gamma, beta, eps, groups)
    return _CACHE[("f", d, eps)]


def _guarded(rows, shape_tail, dtype):
    """(full, view of the first `rows` rows): NaN everywhere; the G rows behind the view must keep their bits"""
    full = torch.full((rows + G,) + tuple(shape_tail), float("nan"), dtype=dtype, device=DEV)
    return full, full[:rows]


def _untouched(*fulls, rows):
    for f in fulls:
        tail = f[rows:]
        ref = torch.full_like(tail, float("nan"))
        it = torch.int16 if f.dtype == torch.bfloat16 else torch.int32
        assert torch.equal(tail.view(it), ref.view(it)), "rows behind the output were written"


def _branch(x, groups, K, seed, scale=0.1):
    """rows of a branch output / A operand that add about `scale` of each row's spread through a [., K] x 0.2 randn product (K = None:
    added directly); zero rows on the constant and one_off families, which must come through unchanged"""
    g = torch.Generator().manual_seed(seed)
    spread = x.float().std(-1)
    for nm in ("constant", "one_off"):
        if nm in groups:
            spread[groups[nm]] = 0.0
    width = x.shape[1] if K is None else K
    amp = scale * spread / (1.0 if K is None else 0.2 * K ** 0.5)
    return (torch.randn(x.shape[0], width, generator=g) * amp[:, None]).to(torch.bfloat16)


# ------------------------------------------------------------------ layernorm_fwd

@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("d", [8, 64, 264, 512, 768, 1032, 2048, 4096])
def test_layernorm_fwd(d, eps):
    inp = _stacked(d, eps)
    R = inp["x"].shape[0]
    yf, y = _guarded(R, (d,), torch.bfloat16)
    mf, mean = _guarded(R, (), torch.float32)
    rf, rstd = _guarded(R, (), torch.float32)
    dh.layernorm_fwd(inp["x"].to(DEV), inp["gamma"].to(DEV), inp["beta"].to(DEV), y, mean, rstd, R, d, eps)
    _untouched(yf, mf, rf, rows=R)
    lr.within_budget_fwd(y, mean, rstd, inp, label=f"layernorm_fwd d={d} eps={eps}")


# ------------------------------------------------------------------ layernorm_bwd

@pytest.mark.parametrize("dyfam", ["unit", "offset"])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("rows", [37, 70])      # 70: a ragged second 32-row block with idle waves
@pytest.mark.parametrize("d", [8, 264, 512, 768, 2048])
def test_layernorm_bwd(d, rows, with_res, dyfam):
    """each family in a launch of its own; mean / rstd are the float64 statistics rounded to fp32, not layernorm_fwd's; the immediate
    and the deferred form (partials left in the workspace, layernorm_bwd_finish_batch) both under the budget"""
    gamma, _ = lr.params(d, seed=d)
    gd = gamma.to(DEV)
    for i, name in enumerate(lr.FAMILIES):
        x = lr.families(name, rows, d, seed=10 * d + i)
        g = torch.Generator().manual_seed(d + rows + i)
        dy = (torch.randn(rows, d, generator=g) + (50 if dyfam == "offset" else 0)).to(torch.bfloat16)   # offset: cancels in dy g - mean(dy g)
        dres = torch.randn(rows, d, generator=g).to(torch.bfloat16) if with_res else None
        _, m64, r64 = lr.ln_fwd64(x, gamma, gamma, 1e-5)
        mean, rstd = m64.float(), r64.float()
        inp = lr.make_inputs_bwd(dy, x, gamma, mean, rstd, dres, {name: torch.arange(rows)})
        args = (dy.to(DEV), x.to(DEV), gd, mean.to(DEV), rstd.to(DEV), None if dres is None else dres.to(DEV))
        nbytes = max(int(dh.layernorm_bwd_workspace_bytes(rows, d)), 256)
        for form in ("immediate", "deferred"):
            dxf, dx = _guarded(rows, (d,), torch.bfloat16)
            dg, db = (torch.full((d,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
            w = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            if form == "immediate":
                dh.layernorm_bwd(*args, dx, dg, db, w, rows, d)
            else:
                dh.layernorm_bwd(*args, dx, None, None, w, rows, d)
                dh.layernorm_bwd_finish_batch([(w, dg, db, rows)], d)
            _untouched(dxf, rows=rows)
            lr.within_budget_bwd(dx, dg, db, inp, label=f"layernorm_bwd {form} d={d} rows={rows} res={int(with_res)} dy={dyfam} {name}")


# ------------------------------------------------------------------ dropout_add_ln

@pytest.mark.parametrize("rate", [0.0, 0.1])
@pytest.mark.parametrize("d", [264, 512])
def test_dropout_add_ln(d, rate):
    """residual holds the family rows, the branch adds about 0.1 of a row's spread (nothing on the constant and one_off rows); the
    LayerNorm outputs against float64 on the stored x_out"""
    base = _stacked(d, 1e-5)
    res, groups, gamma, beta = base["x"], base["groups"], base["gamma"], base["beta"]
    R = res.shape[0]
    a = _branch(res, groups, None, seed=d)
    xf, x_out = _guarded(R, (d,), torch.bfloat16)
    yf, y = _guarded(R, (d,), torch.bfloat16)
    mf, mean = _guarded(R, (), torch.float32)
    rf, rstd = _guarded(R, (), torch.float32)
    dh.dropout_add_ln(a.to(DEV), res.to(DEV), x_out, gamma.to(DEV), beta.to(DEV), y, mean, rstd, R, d, 0x243F6A8885A308D3,
                      dropout_ref.threshold(rate))
    _untouched(xf, yf, mf, rf, rows=R)
    xo = x_out.cpu()
    for nm in ("constant", "one_off"):
        assert torch.equal(xo[groups[nm]], res[groups[nm]]), f"{nm} rows must come through unchanged"
    assert not torch.equal(xo[groups["unit"]], res[groups["unit"]])
    lr.within_budget_fwd(y, mean, rstd, lr.make_inputs_fwd(xo, gamma, beta, 1e-5, groups), label=f"dropout_add_ln d={d} rate={rate}")


# ------------------------------------------------------------------ gemm_nt_ln / gemm_nt_lnbwd (full-row tiles, N = 512)

M_FULL = 200        # one full 160-row tile and a ragged one


def _full_row_x(seed):
    """[200, 512] with the families interleaved over the rows: every 16-row group of both tiles sees each family"""
    key = ("full", seed)
    if key not in _CACHE:
        _CACHE[key] = lr.interleaved(lr.FAMILIES, M_FULL, N_FULL, seed) + lr.params(N_FULL, seed=seed)
    return _CACHE[key]


def _product_operands(K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M_FULL, K, generator=g).to(torch.bfloat16), (0.2 * torch.randn(N_FULL, K, generator=g)).to(torch.bfloat16)


def _gemm_nt_ln(A, Bt, K, gamma, beta, residual, eps=1e-5, ld=None):
    M, N, ld = M_FULL, N_FULL, ld or K
    Cf, C = _guarded(M, (N,), torch.bfloat16)
    Yf, Y = _guarded(M, (N,), torch.bfloat16)
    mf, mean = _guarded(M, (), torch.float32)
    rf, rstd = _guarded(M, (), torch.float32)
    dh.gemm_nt_ln(A.to(DEV), ld, Bt.to(DEV), ld, C, N, M, N, K, gamma.to(DEV), beta.to(DEV), Y, N, mean, rstd,
                  residual=None if residual is None else residual.to(DEV), eps=eps)
    _untouched(Cf, Yf, mf, rf, rows=M)
    return C, Y, mean, rstd


@pytest.mark.parametrize("K", [64, 160])
def test_gemm_nt_ln(K):
    """Y, mean, rstd against float64 LayerNorm of the stored C; the constant and one_off rows have zero A rows and there is no bias,
    so C is exactly the residual there (C's bit-equality with gemm_nt is tests/test_kernels_gpu.py's)"""
    res, groups, gamma, beta = _full_row_x(seed=5)
    g = torch.Generator().manual_seed(K)
    Bt = (0.2 * torch.randn(N_FULL, K, generator=g)).to(torch.bfloat16)
    A = _branch(res, groups, K, seed=K + 1)
    C, Y, mean, rstd = _gemm_nt_ln(A, Bt, K, gamma, beta, res)
    Cc = C.cpu()
    for nm in ("constant", "one_off"):
        assert torch.equal(Cc[groups[nm]], res[groups[nm]]), f"{nm} rows: C must be exactly the residual"
    assert not torch.equal(Cc[groups["unit"]], res[groups["unit"]])
    lr.within_budget_fwd(Y, mean, rstd, lr.make_inputs_fwd(Cc, gamma, beta, 1e-5, groups), label=f"gemm_nt_ln K={K}")
    if K == 64:
        with pytest.raises(dh.DalleHipError):      # k-steps of 32: any other K is refused
            _gemm_nt_ln(A, Bt, 48, gamma, beta, res, ld=64)


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("K", [64, 160])
def test_gemm_nt_lnbwd(K, with_res):
    M, N = M_FULL, N_FULL
    x, groups, gamma, beta = _full_row_x(seed=6)
    A, Bt = _product_operands(K, seed=K + 2)
    dres = torch.randn(M, N, generator=torch.Generator().manual_seed(9)).to(torch.bfloat16) if with_res else None
    _, m64, r64 = lr.ln_fwd64(x, gamma, beta, 1e-5)
    mean, rstd = m64.float(), r64.float()
    dy64 = A.double() @ Bt.double().t()
    # the bf16 product the full-row main loop stores: what the kernel's dgamma / dbeta are sums of
    dyC = _gemm_nt_ln(A, Bt, K, gamma, beta, None)[0].cpu()
    acc = lr.U * K * (A.double().abs() @ Bt.double().abs().t())
    assert bool(((dyC.double() - dy64).abs() <= acc + 2.0 ** -8 * (dy64.abs() + acc)).all()), \
        "the stored product is not the bf16 rounding of an fp32 accumulation of the float64 one"
    inp = lr.make_inputs_bwd(dy64, x, gamma, mean, rstd, dres, groups,
                             dy_emulated=(A.float() @ Bt.float().t()).to(torch.bfloat16), dy_params=dyC)
    dxf, dx = _guarded(M, (N,), torch.bfloat16)
    dg, db = (torch.full((N,), float("nan"), dtype=torch.float32, device=DEV) for _ in range(2))
    part = torch.full((dh.gemm_nt_lnbwd_parts(M) * 2 * N,), float("nan"), dtype=torch.float32, device=DEV)
    dh.gemm_nt_lnbwd(A.to(DEV), K, Bt.to(DEV), K, M, N, K, x.to(DEV), gamma.to(DEV), mean.to(DEV), rstd.to(DEV),
                     None if dres is None else dres.to(DEV), dx, part, dg=dg, db=db)
    _untouched(dxf, rows=M)
    lr.within_budget_bwd(dx, dg, db, inp, label=f"gemm_nt_lnbwd K={K} res={int(with_res)}")


# ------------------------------------------------------------------ ln_gemm_nt (decode prologue)

@pytest.mark.parametrize("K", [64, 512, 2048])
@pytest.mark.parametrize("M", [5, 32])
def test_ln_gemm_nt(M, K):
    """C = LN(X) . Bt^T against LN64(X) . Bt^T in float64 by the row metric; the emulation is bf16(LayerNorm in fp32), an fp32 product,
    a bf16 rounding.  On constant rows LN(X) = beta exactly, so C = bf16(beta . Bt^T) within one bf16 ulp."""
    N, ldx = 48, K + 8
    names = ("rowmix", "constant", "one_off", "offset100")
    x, groups = lr.interleaved(names, M, K, seed=K + M)
    gamma, beta = lr.params(K, seed=K)
    Bt = (0.2 * torch.randn(N, K, generator=torch.Generator().manual_seed(K))).to(torch.bfloat16)
    X = torch.full((M, ldx), float("nan"), dtype=torch.bfloat16)     # columns past K must not be read into the statistics
    X[:, :K] = x
    C = torch.full((M + 1, N + 16), 7.0, dtype=torch.bfloat16, device=DEV)
    dh.ln_gemm_nt(X.to(DEV), ldx, gamma.to(DEV), beta.to(DEV), Bt.to(DEV), K, C, N + 16, M, N, K)
    assert bool((C[M:] == 7.0).all()) and bool((C[:, N:] == 7.0).all()), "wrote outside the [M, N] block"
    got = C[:M, :N].cpu()
    ref = lr.ln_fwd64(x, gamma, beta, 1e-5)[0] @ Bt.double().t()
    emu = (lr.emulated_fwd(x, gamma, beta, 1e-5)[0].float() @ Bt.float().t()).to(torch.bfloat16)
    rmax, rmed, msg = lr.judge_rows(got, ref, emu, "C")
    cref = (beta.double() @ Bt.double().t()).to(torch.bfloat16).double()
    cerr = (got[groups["constant"]].double() - cref[None, :]).abs() / lr.ulp_bf16(cref)[None, :]
    print(f"RATIO ln_gemm_nt M={M} K={K}: C {rmax:.4f} {rmed:.4f} | const {float(cerr.max()):.3g}", flush=True)
    assert msg is None, msg
    assert float(cerr.max()) <= 1.0, "constant rows: C is more than one bf16 ulp off bf16(beta . Bt^T)"
