"""Plain CPU references of LayerNorm forward / backward and the error budget the tests hold the six LayerNorm kernels to (layernorm_fwd,
layernorm_bwd, dropout_add_ln, gemm_nt_ln, gemm_nt_lnbwd, ln_gemm_nt): the LayerNorm counterpart of tests/attention_fwd_ref.py, whose
row metric and margins it imports.  Pure CPU torch.

The kernels take bf16 x [rows, d], bf16 gamma / beta [d], write bf16 y and fp32 mean / rstd [rows]; the backward takes bf16 dy, x,
gamma, fp32 mean / rstd, an optional bf16 residual gradient dres, and writes bf16 dx and fp32 dgamma / dbeta [d].  So do these.

  ln_fwd64   the specification, in float64 on the bf16 inputs:
               mean = sum_j x_j / d;  var = sum_j (x_j - mean)^2 / d  (biased, of the CENTRED row);  rstd = 1 / sqrt(var + eps)  (eps
               inside the root);  y = (x - mean) * rstd * gamma + beta.   eps is the fp32 number the kernels receive (float32(1e-5) is
               not 1e-5, and on a near-constant row eps IS rstd).
  ln_bwd64   xhat = (x - mean) * rstd;  gy = dy * gamma;  dx = rstd * (gy - mean_j(gy) - xhat * mean_j(gy * xhat)) + dres;
             dgamma = sum_rows dy * xhat;  dbeta = sum_rows dy.   mean / rstd are DATA (the given fp32 numbers), so the backward is
             judged apart from the forward.
  emulated_fwd / emulated_bwd   the same formulas in float32, rounded to bf16 exactly where a bf16 LayerNorm rounds: y and dx.  A
             model of bf16 LayerNorm in general, not of one kernel's summation order -- the yardstick of y and dx.  fault= (FAULTS)
             seeds a defect; tests/test_layernorm_ref.py proves the budget rejects each.
  emulated_fwd_lane_order   a second float32 forward that sums the way ln_row (csrc/elementwise.hip) does: element 8 c + j goes to lane
             c mod 64, a lane adds its elements serially, a 6-step xor butterfly combines the lanes.  Proves on the CPU that a correct
             kernel with another summation order than torch's passes.

INPUT FAMILIES (families(name, rows, d, seed), bf16 [rows, d]; FAMILIES):
  unit        randn
  offset100   100 + 2 randn
  offset1000  1000 + 16 randn   (bf16 spacing there is 4..8: the spread survives the rounding)
  tiny        1e-3 randn        (variance 1e-6 < eps)
  huge        3e4 randn
  constant    every element 3.0 (the row sum is exact in fp32 for every d <= 4096)
  one_off     3.0, the LAST column 3 + 2^-6: variance ~ 5e-7, eps decides rstd
  outlier     randn with one element 300 (column (7 r + 3) mod d of row r)
  rowmix      row r = randn * logspace(-3, 3, rows)[r] + linspace(-50, 50, rows)[r]: rows of every scale in one launch

ROW BUDGET of y and dx (within_budget_fwd / within_budget_bwd), per family.  The metric is attention_bwd_ref.row_error taken with
every row as its own group, i.e. ||got - ref||_2 / (1.001 ||ref||_2) per row (a family-wide floor would let the small rows of rowmix
hide behind the large ones); MARGIN_MAX, MARGIN_MED and MEDIAN_FLOOR are the attention references':
    max row error against float64    <= MARGIN_MAX * the emulation's own max
    median row error against float64 <= MARGIN_MED * the emulation's own median, both medians taken no smaller than MEDIAN_FLOOR
DEGENERATE ROWS.  On a constant row x_j - mean is exactly 0 in float64 AND in a correct fp32 kernel (the fp32 row sum of d equal bf16
values is exact here, so is the division), y64 = beta exactly, and the emulation's error is 0: a ratio against it is undefined.  Such
rows (every row with max = min, whatever its family) leave the ratio and are judged element by element,
    |y - beta| <= half a bf16 ulp of beta + |gamma| * rstd64 * ulp32(|x|)
-- one fp32 ulp of slack on the mean (a kernel may multiply by a rounded 1 / d), amplified by gamma * rstd, and the rounding of y.
one_off is NOT degenerate: its emulation error is nonzero, it goes by the row metric like any other family.

DERIVED BOUNDS of the row statistics, u = 2^-24.  L = the longest chain of dependent fp32 additions a kernel makes for one statistic,
counted by reading the kernels:
    ln_row (layernorm_fwd, dropout_add_ln)   8 NC <= 64 serial per lane + 6 butterfly steps                             = 70
    epilogue_ln (gemm_nt_ln)                 variance: 1 centring + 32 serial per lane + 2 lane-group exchanges + 2 over the four waves = 37
                                             (mean: (v0 + v1) + (v2 + v3) added 8 times, + 2 + 2 = 14)
    gemm_ln_nt_skinny_kernel (ln_gemm_nt)    16 * 4 = 64 serial per lane + 2 lane-group exchanges + 8 waves serially    = 74
STAT_DEPTH = 96 covers them with room for one more level.
    |mean - mean64| <= dm = u * (STAT_DEPTH + 2) * mean_j |x_j|                       (L additions + the division, each <= u relative
                                                                                       to a partial sum <= sum_j |x_j|)
    |rstd - rstd64| / rstd64 <= (u * (STAT_DEPTH + 6) + dm^2 / (var64 + eps)) / 2 + 4 u
        (a mean off by dm adds exactly dm^2 to the centred second moment; the centring, the square, L additions, the division and
         the + eps are STAT_DEPTH + 6 roundings of relative size u on non-negative terms; the root halves a relative error; 4 u for
         rsqrtf and a reciprocal)
DERIVED BOUNDS of the parameter gradients (any summation order: the partials go through a workspace and a finish kernel, no
shorter chain is claimed), per column:
    |dgamma - dgamma64| <= u * (rows + 8) * sum_rows |dy * xhat|,     |dbeta - dbeta64| <= u * (rows + 8) * sum_rows |dy|

An `inputs` dict (make_inputs_fwd / make_inputs_bwd) carries the arguments, the row groups (family -> row indices) and caches the
references: they are computed once per input set however many results are judged against them."""
import math

import torch

from attention_bwd_ref import MARGIN_MAX, MARGIN_MED, row_error
from attention_fwd_ref import MEDIAN_FLOOR

FAMILIES = ("unit", "offset100", "offset1000", "tiny", "huge", "constant", "one_off", "outlier", "rowmix")
FAULTS_FWD = ("one_pass_var", "eps_outside", "unbiased", "drop_last_chunk", "mean_bf16")
FAULTS_BWD = ("no_xhat_term", "dgamma_unscaled")
FAULTS = FAULTS_FWD + FAULTS_BWD
U = 2.0 ** -24
STAT_DEPTH = 96


# ------------------------------------------------------------------ inputs

def families(name, rows, d, seed):
    """bf16 [rows, d] of one input family (module docstring)"""
    assert name in FAMILIES, name
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(rows, d, generator=g)
    if name == "unit":
        x = r
    elif name == "offset100":
        x = 100 + 2 * r
    elif name == "offset1000":
        x = 1000 + 16 * r
    elif name == "tiny":
        x = 1e-3 * r
    elif name == "huge":
        x = 3e4 * r
    elif name == "constant":
        x = torch.full((rows, d), 3.0)
    elif name == "one_off":
        x = torch.full((rows, d), 3.0)
        x[:, -1] = 3 + 2.0 ** -6
    elif name == "outlier":
        x = r
        x[torch.arange(rows), (7 * torch.arange(rows) + 3) % d] = 300.0
    else:
        x = r * torch.logspace(-3, 3, rows)[:, None] + torch.linspace(-50, 50, rows)[:, None]
    return x.to(torch.bfloat16)


def stacked(names, rows, d, seed):
    """(x bf16 [len(names) * rows, d], groups): `rows` rows of each family one after the other"""
    x = torch.cat([families(nm, rows, d, seed + i) for i, nm in enumerate(names)])
    return x, {nm: torch.arange(i * rows, (i + 1) * rows) for i, nm in enumerate(names)}


def interleaved(names, M, d, seed):
    """(x bf16 [M, d], groups): row m belongs to family names[m mod len(names)], so every run of len(names) rows sees each"""
    n = len(names)
    x = torch.empty(M, d, dtype=torch.bfloat16)
    groups = {}
    for i, nm in enumerate(names):
        idx = torch.arange(i, M, n)
        x[idx] = families(nm, len(idx), d, seed + i)
        groups[nm] = idx
    return x, groups


def params(d, seed):
    """bf16 (gamma = 1 + 0.1 randn, beta = 0.1 randn)"""
    g = torch.Generator().manual_seed(seed)
    return (1 + 0.1 * torch.randn(d, generator=g)).to(torch.bfloat16), (0.1 * torch.randn(d, generator=g)).to(torch.bfloat16)


def eps32(eps):
    """the fp32 number a kernel receives for eps, as a python float"""
    return float(torch.tensor(float(eps), dtype=torch.float32))


# ------------------------------------------------------------------ float64 specification

def ln_fwd64(x, gamma, beta, eps):
    """(y [rows, d], mean [rows], rstd [rows]) in float64"""
    x, g, b = x.double(), gamma.double(), beta.double()
    mean = x.mean(-1)
    xc = x - mean[:, None]
    rstd = 1.0 / torch.sqrt(xc.pow(2).mean(-1) + eps32(eps))
    return xc * rstd[:, None] * g + b, mean, rstd


def ln_bwd64(dy, x, gamma, mean, rstd, dres=None):
    """(dx [rows, d], dgamma [d], dbeta [d]) in float64; mean / rstd: the given statistics, taken as data"""
    dy, x, g = dy.double(), x.double(), gamma.double()
    xhat = (x - mean.double()[:, None]) * rstd.double()[:, None]
    gy = dy * g
    dx = rstd.double()[:, None] * (gy - gy.mean(-1, keepdim=True) - xhat * (gy * xhat).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.double()
    return dx, (dy * xhat).sum(0), dy.sum(0)


# ------------------------------------------------------------------ float32 emulations

def emulated_fwd(x, gamma, beta, eps, fault=None):
    """(y bf16, mean fp32, rstd fp32) in float32, y rounded to bf16.  fault (one of FAULTS_FWD):
      one_pass_var     var = E[x^2] - mean^2
      eps_outside      rstd = 1 / (sqrt(var) + eps)
      unbiased         var * d / (d - 1)
      drop_last_chunk  the last 8 elements left out of the row sum of the mean
      mean_bf16        the mean rounded to bf16"""
    assert fault is None or fault in FAULTS_FWD
    x, g, b = x.float(), gamma.float(), beta.float()
    d = x.shape[-1]
    e = torch.tensor(float(eps), dtype=torch.float32)
    mean = x[:, :-8].sum(-1) / d if fault == "drop_last_chunk" else x.mean(-1)
    if fault == "mean_bf16":
        mean = mean.to(torch.bfloat16).float()
    xc = x - mean[:, None]
    var = (x * x).mean(-1) - mean * mean if fault == "one_pass_var" else (xc * xc).mean(-1)
    if fault == "unbiased":
        var = var * (d / (d - 1.0))
    rstd = 1.0 / (torch.sqrt(var) + e) if fault == "eps_outside" else torch.rsqrt(var + e)
    return (xc * rstd[:, None] * g + b).to(torch.bfloat16), mean, rstd


def emulated_fwd_lane_order(x, gamma, beta, eps):
    """emulated_fwd with the summation order of ln_row: lane c mod 64 owns the 8-element chunks c, each lane adds its elements
    serially (chunk after chunk), a xor butterfly (32, 16, .., 1) combines the 64 lanes"""
    x, g, b = x.float(), gamma.float(), beta.float()
    rows, d = x.shape
    assert d % 8 == 0
    nch = d // 8
    NC = (nch + 63) // 64
    v = torch.zeros(rows, NC * 64, 8)
    v[:, :nch] = x.view(rows, nch, 8)
    v = v.view(rows, NC, 64, 8)
    valid = (torch.arange(NC * 64) < nch).view(1, NC, 64, 1)
    lanes = torch.arange(64)

    def wave_sum(s):
        for o in (32, 16, 8, 4, 2, 1):
            s = s + s[:, lanes ^ o]
        return s[:, 0]

    def lane_serial(t):
        s = torch.zeros(rows, 64)
        for i in range(NC):
            for j in range(8):
                s = s + t[:, i, :, j]
        return s

    fd = torch.tensor(float(d), dtype=torch.float32)
    mean = wave_sum(lane_serial(v)) / fd
    vc = torch.where(valid, v - mean[:, None, None, None], torch.zeros(()))
    rstd = torch.rsqrt(wave_sum(lane_serial(vc * vc)) / fd + torch.tensor(float(eps), dtype=torch.float32))
    xc = vc.view(rows, NC * 64 * 8)[:, :d]
    return (xc * rstd[:, None] * g + b).to(torch.bfloat16), mean, rstd


def emulated_bwd(dy, x, gamma, mean, rstd, dres=None, fault=None):
    """(dx bf16, dgamma fp32, dbeta fp32) in float32, dx rounded to bf16.  fault (one of FAULTS_BWD):
      no_xhat_term     dx without xhat * mean_j(dy * gamma * xhat)
      dgamma_unscaled  dgamma from x - mean instead of xhat"""
    assert fault is None or fault in FAULTS_BWD
    dy, x, g, mean, rstd = dy.float(), x.float(), gamma.float(), mean.float(), rstd.float()
    xc = x - mean[:, None]
    xhat = xc * rstd[:, None]
    gy = dy * g
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xhat).mean(-1, keepdim=True)
    dx = rstd[:, None] * (gy - s1 - (0 if fault == "no_xhat_term" else xhat * s2))
    if dres is not None:
        dx = dx + dres.float()
    return dx.to(torch.bfloat16), (dy * (xc if fault == "dgamma_unscaled" else xhat)).sum(0), dy.sum(0)


# ------------------------------------------------------------------ bounds

def mean_bound(x):
    """[rows] float64: dm, the derived worst case of |mean - mean64|"""
    return U * (STAT_DEPTH + 2) * x.double().abs().mean(-1)


def rstd_bound(x, eps):
    """[rows] float64: the derived worst case of |rstd - rstd64| / rstd64"""
    x = x.double()
    var = (x - x.mean(-1, keepdim=True)).pow(2).mean(-1)
    return 0.5 * (U * (STAT_DEPTH + 6) + mean_bound(x).pow(2) / (var + eps32(eps))) + 4 * U


def ulp_bf16(v):
    """float64: the spacing of bf16 at |v| (0 at 0)"""
    a = v.double().abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 7), torch.zeros((), dtype=torch.float64))


def ulp32(v):
    a = v.double().abs()
    return torch.where(a > 0, torch.exp2(torch.floor(torch.log2(a.clamp_min(1e-300))) - 23), torch.zeros((), dtype=torch.float64))


def rows_error(got, ref):
    """[rows]: attention_bwd_ref.row_error with every row as its own group"""
    return row_error(got[:, None, :], ref[:, None, :])[:, 0]


def _ratio(a, b):
    return a / b if b > 0 else (0.0 if a == 0 else math.inf)


def judge_rows(got, ref, emu, what, margin_max=MARGIN_MAX, margin_med=MARGIN_MED):
    """the row budget of one group: (max ratio, median ratio, failure message or None)"""
    g = got.detach().cpu()
    if not bool(torch.isfinite(g.float()).all()):
        return math.inf, math.inf, f"{what}: not finite"
    err, eerr = rows_error(g, ref), rows_error(emu, ref)
    gmax, gmed = float(err.max()), max(float(err.median()), MEDIAN_FLOOR)
    emax, emed = float(eerr.max()), max(float(eerr.median()), MEDIAN_FLOOR)
    msg = None
    if gmax > margin_max * emax or gmed > margin_med * emed:
        w = int(err.argmax())
        msg = (f"{what}: worst row {w} of the group: row error {gmax:.4g} (emulation there {float(eerr[w]):.4g}); max {gmax:.4g} vs "
               f"{margin_max} * {emax:.4g}, median {gmed:.4g} vs {margin_med} * {emed:.4g}")
    return _ratio(gmax, emax), gmed / emed, msg


def _finish(kind, label, out, failures, shape):
    if label is not None:
        print(f"RATIO {label}: " + " | ".join(f"{k} " + (" ".join(f"{t:.4f}" for t in v) if isinstance(v, tuple) else f"{v:.3g}")
                                                 for k, v in out.items()), flush=True)
    if failures:
        msg = f"LayerNorm {kind} over its error budget at (rows, d) = {shape}:\n  " + "\n  ".join(failures)
        print(msg, flush=True)
        raise AssertionError(msg)
    return out


# ------------------------------------------------------------------ forward budget

def make_inputs_fwd(x, gamma, beta, eps, groups=None):
    """CPU copies of the forward's arguments; groups: {name: row indices} judged separately (None: all rows as one)"""
    x = x.detach().cpu()
    return dict(x=x, gamma=gamma.detach().cpu(), beta=beta.detach().cpu(), eps=eps,
                groups=groups if groups is not None else {"all": torch.arange(x.shape[0])})


def references_fwd(inp):
    """(y64, mean64, rstd64, emulated y, mean bound, relative rstd bound, constant-row flags), computed once and kept"""
    if "_refs" not in inp:
        x, g, b, eps = inp["x"], inp["gamma"], inp["beta"], inp["eps"]
        y64, m64, r64 = ln_fwd64(x, g, b, eps)
        xf = x.float()
        inp["_refs"] = (y64, m64, r64, emulated_fwd(x, g, b, eps)[0], mean_bound(x), rstd_bound(x, eps),
                        xf.max(-1).values == xf.min(-1).values)
    return inp["_refs"]


def within_budget_fwd(y, mean, rstd, inp, margin_max=MARGIN_MAX, margin_med=MARGIN_MED, label=None):
    """y bf16 [rows, d], mean / rstd fp32 [rows] (None: not judged) of a LayerNorm forward of inp.  Asserts the row budget of y per
    group, the constant-row rule, and the derived bounds of mean and rstd (module docstring); returns dict(y=(worst max ratio, worst
    median ratio over the groups), const=worst |y - beta| over its bound, mean=, rstd=worst error over its bound); with a label prints
    them as a RATIO line before it asserts."""
    y64, m64, r64, ey, mb, rb, const = references_fwd(inp)
    out, failures = {}, []
    if y is not None:
        yc = y.detach().cpu()
        worst = [0.0, 0.0]
        for name, idx in inp["groups"].items():
            live = idx[~const[idx]]
            if len(live):
                rmax, rmed, msg = judge_rows(yc[live], y64[live], ey[live], f"y[{name}]", margin_max, margin_med)
                worst = [max(worst[0], rmax), max(worst[1], rmed)]
                if msg:
                    failures.append(msg)
        out["y"] = tuple(worst)
        if bool(const.any()):
            beta, gamma = inp["beta"].double(), inp["gamma"].double()
            xa = inp["x"][const].double().abs().max(-1).values
            bound = 0.5 * ulp_bf16(beta)[None, :] + gamma.abs()[None, :] * (r64[const] * ulp32(xa))[:, None]
            err = (yc[const].double() - beta[None, :]).abs()
            err = torch.nan_to_num(err, nan=math.inf)
            ok = err <= bound
            out["const"] = float(torch.where(err > 0, err / bound, torch.zeros((), dtype=torch.float64)).max())
            if not bool(ok.all()):
                failures.append(f"y on constant rows: {int((~ok).sum())} elements off beta by more than half a bf16 ulp + |gamma| rstd ulp32(x); "
                                f"worst |y - beta| = {float(torch.nan_to_num(err, nan=math.inf).max()):.4g}")
    for nm, got, ref, bound in (("mean", mean, m64, mb), ("rstd", rstd, r64, rb * r64)):
        if got is None:
            continue
        gt = got.detach().cpu().double()
        if not bool(torch.isfinite(gt).all()):
            failures.append(f"{nm}: not finite")
            continue
        err = (gt - ref).abs()
        ratio = torch.where(err > 0, err / bound, torch.zeros((), dtype=torch.float64))
        out[nm] = float(ratio.max())
        if not bool((err <= bound).all()):
            w = int(ratio.argmax())
            failures.append(f"{nm}: row {w}: {float(gt[w]):.9g} vs float64 {float(ref[w]):.9g}, error {float(err[w]):.4g} = "
                            f"{out[nm]:.3g} x its bound {float(bound[w]):.4g}")
    return _finish("forward", label, out, failures, tuple(inp["x"].shape))


# ------------------------------------------------------------------ backward budget

def make_inputs_bwd(dy, x, gamma, mean, rstd, dres=None, groups=None, dy_emulated=None, dy_params=None):
    """CPU copies of the backward's arguments.  dy: what the specification of dx takes (bf16, or the float64 product of a fused
    kernel); dy_emulated: what the emulation takes (default dy); dy_params: what the specification and the bounds of dgamma / dbeta
    take (default dy)."""
    c = lambda t: None if t is None else t.detach().cpu()
    x = c(x)
    return dict(dy=c(dy), x=x, gamma=c(gamma), mean=c(mean), rstd=c(rstd), dres=c(dres),
                dy_emulated=c(dy if dy_emulated is None else dy_emulated), dy_params=c(dy if dy_params is None else dy_params),
                groups=groups if groups is not None else {"all": torch.arange(x.shape[0])})


def references_bwd(inp):
    """(dx64, dgamma64, dbeta64, emulated dx, dgamma bound, dbeta bound), computed once and kept"""
    if "_refs" not in inp:
        x, g, mean, rstd, dres = (inp[k] for k in ("x", "gamma", "mean", "rstd", "dres"))
        dx64 = ln_bwd64(inp["dy"], x, g, mean, rstd, dres)[0]
        dyp = inp["dy_params"].double()
        _, dg64, db64 = ln_bwd64(dyp, x, g, mean, rstd)
        xhat = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
        c = U * (x.shape[0] + 8)
        inp["_refs"] = (dx64, dg64, db64, emulated_bwd(inp["dy_emulated"], x, g, mean, rstd, dres)[0],
                        c * (dyp * xhat).abs().sum(0), c * dyp.abs().sum(0))
    return inp["_refs"]


def within_budget_bwd(dx, dg, db, inp, margin_max=MARGIN_MAX, margin_med=MARGIN_MED, label=None):
    """dx bf16 [rows, d], dg / db fp32 [d] (None: not judged) of a LayerNorm backward of inp.  Asserts the row budget of dx per group
    and the derived bounds of dgamma / dbeta; returns dict(dx=(worst max ratio, worst median ratio), dg=, db=worst error over bound)."""
    dx64, dg64, db64, edx, gb, bb = references_bwd(inp)
    out, failures = {}, []
    if dx is not None:
        dc = dx.detach().cpu()
        worst = [0.0, 0.0]
        for name, idx in inp["groups"].items():
            rmax, rmed, msg = judge_rows(dc[idx], dx64[idx], edx[idx], f"dx[{name}]", margin_max, margin_med)
            worst = [max(worst[0], rmax), max(worst[1], rmed)]
            if msg:
                failures.append(msg)
        out["dx"] = tuple(worst)
    for nm, got, ref, bound in (("dg", dg, dg64, gb), ("db", db, db64, bb)):
        if got is None:
            continue
        gt = got.detach().cpu().double()
        if not bool(torch.isfinite(gt).all()):
            failures.append(f"{nm}: not finite")
            continue
        err = (gt - ref).abs()
        ratio = torch.where(err > 0, err / bound, torch.zeros((), dtype=torch.float64))
        out[nm] = float(ratio.max())
        if not bool((err <= bound).all()):
            w = int(ratio.argmax())
            failures.append(f"{nm}: column {w}: {float(gt[w]):.9g} vs float64 {float(ref[w]):.9g}, error {float(err[w]):.4g} = "
                            f"{out[nm]:.3g} x its bound {float(bound[w]):.4g}")
    return _finish("backward", label, out, failures, tuple(inp["x"].shape))
