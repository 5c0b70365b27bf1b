"""The KL term and the codebook statistics of the discrete VAE (dalle-mtf_amd/csrc/vae.hip: dmi_codebook_kl_fwd,
dmi_gumbel_softmax_bwd_kl, dmi_codebook_usage) restated on the CPU: the float64 specification, an fp32 restatement in numpy with a
selectable summation order, and the error bounds the GPU tests use.  CPU only (numpy).

Specification, per row m of the fp32 logits l [M, T] (no noise, no temperature):
    lse_m = logsumexp_k l[m,k]        q[m,k] = exp(l[m,k] - lse_m)        ln q[m,k] = l[m,k] - lse_m
    e_m = sum_k q ln q  (q = 0 contributes 0)        KL_m = e_m + ln T        KL = (1/M) sum_m KL_m
    dlogits[m,j] = (1/tau) p_j (dy_j - sum_k dy_k p_k) + (beta_t / M) q_j (ln q_j - e_m)       (p = y_soft of the Gumbel forward)
    qsum[k] = sum_m q[m,k]            counts[k] = #{m : index[m] == k}

Error model (u = 2^-24, the fp32 unit roundoff; every bound is first order in u and evaluated on float64 quantities of the
specification -- no measured constant).  The fp32 computation is
    mx = max_k l_k (exact);  d_k = fl(l_k - mx);  t_k = exp(d_k);  s = sum t_k;  a = sum t_k d_k;  ls = log(s)
    lse = fl(mx + ls);  e = fl(fl(a / s) - ls);  KL_m = fl(e + fl(ln T));  KL = fl(sum_m KL_m) * fl(1/M)
with the sums in ANY order (a sum of n terms of one sign has relative error <= (n - 1) u whatever the order).  exp(x) is the
hardware's exp2 of fl(x fl(log2 e)), as in gumbel_fwd_kernel: the rounding of the constant and of the product move the result by
|x| u relative each.  exp2 (v_exp_f32) and the library logf are documented to 1 ulp, and one ulp is at most 2 u relative:
EXP_U = LOG_U = 2, in units of u.
With q the exact posterior, A1 = sum_k q_k |d_k| and A2 = sum_k q_k d_k^2:
  * s: t_k carries the rounding of d_k, of log2 e and of their product (relative u |d_k| on exp each) and the exp2, then the sum:
        rel_s = (T + EXP_U + 3 A1) u
  * lse: log(s) moves by rel_s, plus the log's own ulps at |ls|, plus the final rounding at the magnitude of lse:
        B_lse = rel_s + LOG_U u |ls| + u |lse|
  * e: the terms t_k d_k are all <= 0: the product (1 u), t_k as above (EXP_U + 3 |d_k|) u, the rounding of the factor d_k (1 u),
    the sum (T u); dividing by s adds rel_s and one rounding, both on A1; then ls (as above) and the final subtraction at |e|:
        B_e = u ((T + EXP_U + 3) A1 + 3 A2) + rel_s (A1 + 1) + LOG_U u |ls| + u |e|
  * KL: B_KLm = B_e + u ln T + u |KL_m|; the mean goes through an any-order sum of M terms and two roundings for 1/M:
        B_KL = mean_m B_KLm + (M + 2) u mean_m |KL_m|
  * dlogits: ln q is recomputed as fl(l - lse) from the STORED lse: |d lnq| <= B_lse + u |ln q| =: D; q = exp(that): relative
    D + (EXP_U + 2 |ln q|) u =: Q (the constant and the product); w = fl(lnq - e): D + B_e + u |w|; c = fl(beta_t / M) and two products: 3 u.  The Gumbel term is the existing
    kernel's (bf16 x bf16 products exact, an any-order dot, then four roundings); one more rounding for the final add:
        E_k = (beta_t / M) q ((Q + 3 u) |w| + D + B_e + u |w|)
        E_g = (1/tau) p u ((T + 2) S + 4 (|dy| + |dot|)),   S = sum_k |dy_k p_k|
        E = E_g + E_k + u |r|,        B_dlogits = E + half a bf16 ulp at (|r| + E) + (1/tau + beta_t / M) 2^-126  (the denormal floor)
  * qsum: q as in dlogits, then an any-order sum of M non-negative terms (the two stages are one such order):
        B_qsum[k] = sum_m q[m,k] Q[m,k] + M u qsum[k] + M 2^-126
Every bound gets + 2^-126 T where a sum of T possibly flushed terms enters."""
import numpy as np

U = 2.0 ** -24
EXP_U = LOG_U = 2          # 1 ulp (documented for v_exp_f32 and logf) in units of u
TINY = 2.0 ** -126

FAULTS = ("no_ln_t", "no_e", "over_mt", "q_at_temp")       # seeded faults the bounds must catch (tests/test_vae_kl.py)


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def bf16_ulp(x):
    """one bf16 ulp at |x| (7 explicit mantissa bits); the ulp of the smallest normal below it"""
    e = np.floor(np.log2(np.maximum(np.abs(_f64(x)), TINY)))
    return 2.0 ** (e - 7)


def round_bf16(x):
    """fp32 array -> the nearest bf16 value (ties to even), as fp32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


# ------------------------------------------------------------------ float64 specification
def kl_spec(logits):
    """-> dict(lse [M], q [M,T], lnq [M,T], e [M], klm [M], kl) in float64"""
    l = _f64(logits)
    mx = l.max(axis=-1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(l - mx).sum(axis=-1))
    lnq = l - lse[:, None]
    q = np.exp(lnq)
    e = np.where(q > 0, q * lnq, 0.0).sum(axis=-1)
    klm = e + np.log(float(l.shape[1]))
    return dict(lse=lse, q=q, lnq=lnq, e=e, klm=klm, kl=float(klm.mean()))


def bwd_terms(dy, y_soft, logits):
    """what the gradient and its bound are made of, computed once per input: G = p (dy - sum dy p), K = q (ln q - e) / M, and the
    matching parts Eg, Ek of the fp32 error (module docstring), so that for every (tau, beta_t)
        dlogits = G / tau + beta_t K,        E = Eg / tau + beta_t Ek + u |dlogits|"""
    a, p = _f64(dy), _f64(y_soft)
    s = kl_spec(logits)
    M, T = s["q"].shape
    dot = (a * p).sum(axis=-1, keepdims=True)
    w = s["lnq"] - s["e"][:, None]
    D = lse_bound(logits)[:, None] + U * np.abs(s["lnq"])
    Q = D + (EXP_U + 2.0 * np.abs(s["lnq"])) * U
    Ek = s["q"] / M * ((Q + 3 * U) * np.abs(w) + D + e_bound(logits)[:, None] + U * np.abs(w))
    S = np.abs(a * p).sum(axis=-1, keepdims=True)
    Eg = p * U * ((T + 2) * S + 4 * (np.abs(a) + np.abs(dot)))
    return dict(G=p * (a - dot), K=s["q"] * w / M, Eg=Eg, Ek=Ek, M=M)


def dlogits_from_terms(t, temperature, beta_t):
    """-> (dlogits, its bound) in float64 for the fp32 temperature and weight the kernel is given"""
    it, b = 1.0 / float(np.float32(temperature)), float(np.float32(beta_t))
    r = it * t["G"] + b * t["K"]
    E = it * t["Eg"] + b * t["Ek"] + U * np.abs(r)
    return r, E + 0.5 * bf16_ulp(np.abs(r) + E) + (it + b / t["M"]) * TINY


def dlogits_spec(dy, y_soft, logits, temperature, beta_t):
    """(1/tau) p (dy - sum dy p) + (beta_t / M) q (ln q - e), tau and beta_t the fp32 values the kernel is given"""
    return dlogits_from_terms(bwd_terms(dy, y_soft, logits), temperature, beta_t)[0]


def qsum_spec(logits):
    return kl_spec(logits)["q"].sum(axis=0)


def counts_spec(index, T):
    idx = np.asarray(index).astype(np.int64)
    return np.bincount(idx[(idx >= 0) & (idx < T)], minlength=T).astype(np.int64)


def stats_spec(logits, index):
    """what DiscreteVAE.codebook_stats() returns, from the float64 posterior and the picks"""
    s = kl_spec(logits)
    M, T = s["q"].shape

    def perp(w):
        p = _f64(w) / _f64(w).sum()
        p = p[p > 0]
        return float(np.exp(-(p * np.log(p)).sum()))
    c = counts_spec(index, T)
    used = int((c > 0).sum())
    return dict(kl=s["kl"], perplexity_soft=perp(s["q"].sum(axis=0)), perplexity_hard=perp(c), codes_used=used, codes_used_frac=used / T)


# ------------------------------------------------------------------ fp32 restatement
def _sum32(x, order, axis=-1):
    """fp32 sum along `axis`: order 0 = numpy's pairwise sum of the terms as they stand; order 1 = strictly left to right over the
    REVERSED terms (cumsum is sequential)"""
    x = np.asarray(x, np.float32)
    if order == 0:
        return x.sum(axis=axis, dtype=np.float32)
    x = np.flip(x, axis=axis)
    return np.take(np.cumsum(x, axis=axis, dtype=np.float32), -1, axis=axis)


def _exp32(x):
    """exp as the kernels form it: exp2 of the fp32 product x log2(e)"""
    return np.exp2(np.asarray(x, np.float32) * np.float32(1.4426950408889634))


def kl_fwd_f32(logits, order=0, fault=None):
    """-> (rowstat [M, 2] = (lse, e), kl) computed in fp32 throughout"""
    f32 = np.float32
    l = np.asarray(logits, f32)
    M, T = l.shape
    mx = l.max(axis=-1, keepdims=True)
    d = l - mx
    t = _exp32(d)
    s, a = _sum32(t, order), _sum32(t * d, order)
    ls = np.log(s)
    lse = mx[:, 0] + ls
    e = a / s - ls
    klm = e if fault == "no_ln_t" else e + f32(np.log(float(T)))
    kl = f32(_sum32(klm, order, axis=0) * (f32(1.0) / f32(M)))
    return np.stack([lse, e], axis=1).astype(f32), float(kl)


def bwd_kl_f32(dy, y_soft, logits, rowstat, temperature, beta_t, order=0, fault=None):
    """-> dlogits as bf16 values (float64 array); dy, y_soft: bf16-valued arrays"""
    f32 = np.float32
    a, p, l = np.asarray(dy, f32), np.asarray(y_soft, f32), np.asarray(logits, f32)
    M, T = l.shape
    it = f32(1.0) / f32(temperature)
    dot = _sum32(a * p, order)[:, None]
    g = it * p * (a - dot)
    cw = f32(beta_t) / f32(M)
    if fault == "over_mt":
        cw = cw / f32(T)
    lq = l - rowstat[:, 0:1]
    q = _exp32(lq)
    if fault == "q_at_temp":
        z = (l - l.max(axis=-1, keepdims=True)) * it
        q = _exp32(z) / _sum32(_exp32(z), order)[:, None]
    w = lq if fault == "no_e" else lq - rowstat[:, 1:2]
    out = g + cw * q * w if cw != 0 else g
    return round_bf16(out.astype(f32)).astype(np.float64)


def qsum_f32(logits, rowstat, order=0):
    l = np.asarray(logits, np.float32)
    return _sum32(_exp32(l - rowstat[:, 0:1]), order, axis=0)


# ------------------------------------------------------------------ bounds (module docstring)
def _row_terms(logits):
    l = _f64(logits)
    T = l.shape[1]
    s = kl_spec(l)
    d = l - l.max(axis=-1, keepdims=True)
    ls = np.log(np.exp(d).sum(axis=-1))
    A1 = (s["q"] * np.abs(d)).sum(axis=-1)
    A2 = (s["q"] * d * d).sum(axis=-1)
    rel_s = (T + EXP_U + 3.0 * A1) * U
    return s, T, ls, A1, A2, rel_s


def lse_bound(logits):
    s, T, ls, A1, A2, rel_s = _row_terms(logits)
    return rel_s + LOG_U * U * np.abs(ls) + U * np.abs(s["lse"]) + T * TINY


def e_bound(logits):
    s, T, ls, A1, A2, rel_s = _row_terms(logits)
    return U * ((T + EXP_U + 3) * A1 + 3.0 * A2) + rel_s * (A1 + 1.0) + LOG_U * U * np.abs(ls) + U * np.abs(s["e"]) + T * TINY


def kl_bound(logits):
    s = kl_spec(logits)
    M, T = s["q"].shape
    bm = e_bound(logits) + U * np.log(float(T)) + U * np.abs(s["klm"])
    return float(bm.mean() + (M + 2) * U * np.abs(s["klm"]).mean() + TINY)


def dlogits_bound(dy, y_soft, logits, temperature, beta_t):
    return dlogits_from_terms(bwd_terms(dy, y_soft, logits), temperature, beta_t)[1]


def qsum_bound(logits):
    s = kl_spec(logits)
    M = s["q"].shape[0]
    D = lse_bound(logits)[:, None] + U * np.abs(s["lnq"])
    Q = D + (EXP_U + 2.0 * np.abs(s["lnq"])) * U
    return (s["q"] * Q).sum(axis=0) + M * U * s["q"].sum(axis=0) + M * TINY


# ------------------------------------------------------------------ inputs
FAMILIES = ("normal", "peaked", "constant", "spike60", "shifted")


def family(name, M, T, seed=0):
    """fp32 logits [M, T]: normal x 1; normal x 8 (peaked); a constant row (q exactly uniform: KL = 0, zero KL gradient, the absolute
    part of the bounds decides); one logit 60 above the rest (the others' q underflow in the products); normal + 1000 (shift
    invariance at a magnitude where fp32 absolute error shows)"""
    g = np.random.default_rng([seed, M, T, FAMILIES.index(name)])
    l = g.standard_normal((M, T))
    if name == "peaked":
        l = l * 8.0
    elif name == "constant":
        l = np.full((M, T), 0.375) + g.integers(-2, 3, size=(M, 1))
    elif name == "spike60":
        l[np.arange(M), g.integers(0, T, size=M)] = l.max(axis=-1) + 60.0
    elif name == "shifted":
        l = l + 1000.0
    return l.astype(np.float32)


def bwd_inputs(M, T, temperature, logits, seed=0):
    """bf16-valued (dy, y_soft) as fp32 arrays: y_soft = a Gumbel softmax of the logits at `temperature`, dy ~ 0.01 N(0, 1)"""
    g = np.random.default_rng([seed, M, T, 77])
    u = g.uniform(1e-9, 1.0, (M, T))
    z = (_f64(logits) - np.log(-np.log(u))) / float(temperature)
    z -= z.max(axis=-1, keepdims=True)
    p = np.exp(z)
    p /= p.sum(axis=-1, keepdims=True)
    return round_bf16((g.standard_normal((M, T)) * 0.01).astype(np.float32)), round_bf16(p.astype(np.float32))


# the engine case of "the KL term lowers the KL": the smallest VAE the kernels allow, soft Gumbel at temperature 1, beta = 5
SIGN_CASE = dict(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch=2, beta=5.0, lr=1e-3, steps=20, param_seed=4321,
                 image_seed=0, noise_seed=7)
