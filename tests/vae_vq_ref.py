"""The vector-quantised bottleneck of the discrete VAE (dalle-mtf_amd/csrc/vae.hip: dmi_vq_half_norms, dmi_vq_assign,
dmi_vq_scores_bias, dmi_vq_loss, dmi_vq_bwd_x, dmi_vq_codebook_grad, dmi_vq_gather) restated on the CPU: the float64 specification,
the error bounds the GPU tests use, and the input families.  CPU only (numpy).

Specification.  X bf16-valued [M, D]; C = codebook_t bf16-valued [T, D] (code k = row k, the transpose of codebook/codebook);
d the decoder's gradient with respect to its input; beta the commitment weight:
    h[k] = 1/2 sum_j C[k,j]^2          s[m,k] = sum_j X[m,j] C[k,j] - h[k]          (arg max_k s = arg min_k ||X[m] - C[k]||^2)
    idx[m] = lowest k among the maxima of the kernel's own fp32 scores            xq[m,:] = C[idx[m],:]
    Lq = (1/(M D)) sum_m ||X[m] - xq[m]||^2        loss = recon + (1 + beta) Lq
    dX[m,:] = bf16(d[m,:] + a (X[m,:] - xq[m,:])),  a = 2 beta / (M D)
    dC[k,:] = (2/(M D)) sum_{m: idx[m] = k} (C[k,:] - X[m,:])        (0 for a code nobody picked; nothing from the decoder)
That dX and dC are the gradient of  recon(x + (e - x).detach()) + mean((x.detach() - e)^2) + beta mean((x - e.detach())^2)  is checked
with autograd in tests/test_vae_vq.py.

Error model (u = 2^-24; first order in u; every bound is evaluated on float64 quantities of the specification -- no measured
constant).
  * score.  The products of two bf16 values are exact in fp32 (8 x 8 significant bits).  The kernel adds the D products into an fp32
    accumulator (v_mfma_f32_16x16x32_bf16; whatever the order inside the instruction, a sum of n terms loses at most (n - 1) u times
    the sum of their magnitudes) and subtracts h[k], which itself is a sum of D exact squares halved exactly: D - 1 additions for the
    dot product, at most D - 1 for h, one subtraction -- at most D + 1 roundings act on any one term, so
        |s32[m,k] - s[m,k]| <= (D + 2) u (sum_j |X[m,j] C[k,j]| + h[k])  =:  e[m,k]        (one more u for the rounding of the result)
    The pick compares two such scores, so with  bound_m = 2 (D + 2) u max_k (sum_j |X[m,j] C[k,j]| + h[k]):
        the float64 score of the picked code is within bound_m of the float64 maximum (every row), and
        a row whose float64 best and runner-up VALUES differ by more than bound_m is decided: idx must be the float64 arg-max.
    The winning score the kernel returns is one such score: within bound_m / 2.
    The exact-fp32 tokenising path multiplies fp32 values: one more rounding per product, (D + 3) u in place of (D + 2) u.
  * h from bf16: a lane adds the 8 exact squares of its 16-byte piece (the first addition to 0 is exact), six wave_sum levels, an exact
    halving: at most 14 u h[k].  From the fp32 masters: one rounding per square, D additions: (D + 1) u h[k].
  * dmi_vq_scores_bias is one fp32 subtraction: the GPU test asks for the bits of numpy's.
  * Lq: all terms are >= 0, so the relative error is the number of roundings on the longest path: the difference (2 u on its square),
    the square, the thread's chain of 8 L additions (L = ceil(ceil(M D / 8) / (1024 blocks x 256 threads)) pieces of 8), six wave_sum
    levels, two for the four waves, then dmi_sum_f32 over the 1024 partials (3 + 2 in the thread, 6 wave_sum levels, 16 in the last
    thread), the scale 1/(M D) and its own rounding:
        |Lq32 - Lq| <= (8 L + 40) u Lq
  * dX: a = fp32(2 beta / (M D)) (1 u), the difference, the product and the sum (3 u) act on |d| + a |x - xq|, then one bf16 rounding:
        E = 4 u (|d| + a |x - xq|),   bound = E + half a bf16 ulp at (|dX| + E)
  * dC element (k, j) with n_k rows: each term C - X is one rounding, the chain n_k - 1 additions, the scale 2/(M D) and its rounding:
    at most n_k + 2 roundings; the bound the tests use is the looser
        (n_k + 4) u (2/(M D)) (sum_{m in k} |X[m,j]| + n_k |C[k,j]|);      n_k = 0: exactly 0."""
import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126

FAMILIES = ("normal", "cluster", "bignorm", "dup", "neartie")
CAPPED = ("normal", "cluster", "bignorm")      # families whose undecided rows are capped (at most 5 % of a case)
CAP = 0.05


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def bf16_ulp(x):
    e = np.floor(np.log2(np.maximum(np.abs(_f64(x)), TINY)))
    return 2.0 ** (e - 7)


def round_bf16(x):
    """fp32 array -> the nearest bf16 value (ties to even), as fp32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------ float64 specification
def half_norms(C):
    C = _f64(C)
    return 0.5 * (C * C).sum(axis=1)


def assign_spec(X, C, products_exact=True):
    """-> dict(s [M, T] float64 scores, idx [M] the float64 arg-max (lowest index), best [M], gap [M] = best - runner-up VALUE (inf for
    T == 1; 0 when two codes tie exactly), bound [M] = bound_m, decided [M])"""
    X, C = _f64(X), _f64(C)
    D = X.shape[1]
    h = half_norms(C)
    s = X @ C.T - h[None, :]
    mag = np.abs(X) @ np.abs(C).T + h[None, :]
    bound = 2.0 * (D + (2 if products_exact else 3)) * U * mag.max(axis=1)
    idx = s.argmax(axis=1)
    best = s.max(axis=1)
    if s.shape[1] > 1:
        t = s.copy()
        t[np.arange(s.shape[0]), idx] = -np.inf
        gap = best - t.max(axis=1)
    else:
        gap = np.full(s.shape[0], np.inf)
    return dict(s=s, idx=idx, best=best, gap=gap, bound=bound, decided=gap > bound, h=h)


D_VALUES = (64, 128, 512)        # one k-chunk of 64, two, the largest
T_VALUES = (64, 576, 4096)       # one wave's column tile, a count that is no power of two (two and a quarter block tiles), the largest
M_VALUES = (1, 7, 1030)          # a lone row, a ragged block, seventeen blocks with a ragged last one


def check_assign(spec, idx, score=None):
    """the three criteria of the module docstring on a kernel's picks -> (worst deficit / bound, undecided fraction, worst winning-score
    error / (bound / 2)); raises AssertionError on a violation"""
    s, bound = spec["s"], spec["bound"]
    idx = np.asarray(idx).astype(np.int64)
    M, T = s.shape
    assert idx.shape == (M,) and (idx >= 0).all() and (idx < T).all(), "index out of range"
    picked = s[np.arange(M), idx]
    deficit = spec["best"] - picked
    assert (deficit <= bound).all(), ("picked score below the maximum by more than bound_m", int(np.argmax(deficit / bound)), float(np.max(deficit / bound)))
    dec = spec["decided"]
    assert (idx[dec] == spec["idx"][dec]).all(), ("a decided row picked another code", np.flatnonzero(dec & (idx != spec["idx"]))[:4].tolist())
    w = 0.0
    if score is not None:
        err = np.abs(_f64(score) - picked)
        assert (err <= bound / 2).all(), ("winning score off by more than bound_m / 2", float(np.max(err / (bound / 2))))
        w = float(np.max(err / (bound / 2)))
    return float(np.max(deficit / bound)), float(1.0 - dec.mean()), w


def lq_spec(X, xq):
    X, xq = _f64(X), _f64(xq)
    return float(((X - xq) ** 2).sum() / X.size)


def lq_bound(X, xq):
    n = X.size
    L = -(-(-(-n // 8)) // (1024 * 256))
    return (8 * L + 40) * U * lq_spec(X, xq) + TINY


def dx_spec(d, X, xq, beta):
    """-> (dX before the bf16 rounding, its bound) in float64; beta as the fp32 value the kernel is given"""
    d, X, xq = _f64(d), _f64(X), _f64(xq)
    a = 2.0 * float(np.float32(beta)) / X.size
    want = d + a * (X - xq)
    E = 4.0 * U * (np.abs(d) + a * np.abs(X - xq))
    return want, E + 0.5 * bf16_ulp(np.abs(want) + E) + TINY


def dc_spec(X, idx, C):
    """-> (dC [T, D] in the codebook_t layout, its bound); the [D, T] gradient buffer is the transpose"""
    X, C = _f64(X), _f64(C)
    idx = np.asarray(idx).astype(np.int64)
    M, D = X.shape
    T = C.shape[0]
    n = np.bincount(idx, minlength=T).astype(np.float64)
    S, A = np.zeros((T, D)), np.zeros((T, D))
    np.add.at(S, idx, X)
    np.add.at(A, idx, np.abs(X))
    sc = 2.0 / (M * D)
    want = sc * (n[:, None] * C - S)
    bound = (n[:, None] + 4.0) * U * sc * (A + n[:, None] * np.abs(C))
    bound[n == 0] = 0.0
    return want, bound


def h_bound(C, from_f32=False):
    D = np.asarray(C).shape[1]
    return ((D + 1) if from_f32 else 14) * U * half_norms(C) + TINY


# ------------------------------------------------------------------ the specification as an autograd graph (torch, float64)
def autograd_grads(X, C, W, beta):
    """gradients of  recon_stub(x + (e - x).detach()) + mean((x.detach() - e)^2) + beta mean((x - e.detach())^2)  with respect to x and
    C, e = C[idx]; recon_stub(z) = sum(z * W) -> (dX, dC [T, D], d = d recon / d z)"""
    import torch
    x = torch.tensor(_f64(X), requires_grad=True)
    c = torch.tensor(_f64(C), requires_grad=True)
    idx = torch.tensor(assign_spec(X, C)["idx"])
    e = c[idx]
    z = x + (e - x).detach()
    loss = (z * torch.tensor(_f64(W))).sum() + ((x.detach() - e) ** 2).mean() + beta * ((x - e.detach()) ** 2).mean()
    loss.backward()
    return x.grad.numpy(), c.grad.numpy(), _f64(W)


# ------------------------------------------------------------------ inputs
# seeds for which the float64 reference keeps a capped family's undecided rows at or under CAP (checked in tests/test_vae_vq.py)
SEEDS = {("bignorm", 512, 4096, 1030): 1}


def family(name, M, D, T, seed=None):
    """bf16-valued fp32 (X [M, D], C [T, D]).  normal: X ~ N(0, 1), codes 0.1 N(0, 1).  cluster: X = a code + 0.01 N(0, 1), the trained
    regime.  bignorm: every seventh code scaled by 8, so that h decides.  dup: the upper half of the codebook repeats the lower half
    (every pick must be < T / 2).  neartie: codes come in pairs one bf16 ulp apart in four channels, X next to a pair."""
    if seed is None:
        seed = SEEDS.get((name, D, T, M), 0)
    g = np.random.default_rng([seed, M, D, T, FAMILIES.index(name)])
    C = round_bf16((0.1 * g.standard_normal((T, D))).astype(np.float32))
    X = g.standard_normal((M, D))
    if name == "cluster":
        X = C[g.integers(0, T, size=M)] + 0.01 * g.standard_normal((M, D))
    elif name == "bignorm":
        C[::7] = round_bf16(C[::7] * np.float32(8.0))
    elif name == "dup":
        C[T // 2:] = C[:T // 2]
    elif name == "neartie":
        ch = g.integers(0, D, size=(T // 2, 4))
        C[1::2] = C[0::2]
        rows = np.arange(T // 2)[:, None]
        v = C[1::2][rows, ch]
        C[2 * rows + 1, ch] = (v.astype(np.float64) + bf16_ulp(v)).astype(np.float32)     # the next bf16 value: exact in fp32
        X = C[2 * g.integers(0, T // 2, size=M)] + 0.01 * g.standard_normal((M, D))
    return round_bf16(X.astype(np.float32)), C


def bwd_inputs(X, C, seed=0):
    """bf16-valued d ~ 1e-4 N(0, 1) (the size of a decoder gradient under the 1/(N C) of the MSE), as fp32"""
    g = np.random.default_rng([seed, X.shape[0], X.shape[1], 99])
    return round_bf16((1e-4 * g.standard_normal(X.shape)).astype(np.float32))
