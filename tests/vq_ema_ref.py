"""EMA codebook updates and dead-code restarts of the vector-quantised VAE (dmi_vq_cluster_sums, dmi_vq_ema_step) restated in numpy from
their specification (DESIGN.md §4 "VAE: EMA codebook and restarts"), not from the kernels.  CPU only.

State per code k: N[k] fp32, S[k][0..D) fp32 ([T, D]), idle[k] int32; one counter restarts.  Initial: N = 1, S[k] = C[:,k], idle = 0.
A training step with x bf16-valued [M, D] and idx int32 [M]:
  1. n[k] = #{m : idx[m] = k} (exact), s[k][c] = sum_{idx[m]=k} x[m][c] in fp32, some fixed order.
  2. g = fp32(gamma), w = fp32(1 - gamma) (the difference in double), every product rounded on its own:
       n[k] > 0:  N' = g N + w float(n),  S' = g S + w s,  C[:,k] = S' / N',  idle = 0
       n[k] = 0:  N' = g N,  S' = g S,  idle += 1,  C[:,k] keeps its bits
  3. R > 0, every k with idle[k] >= R after 2:  r = splitmix64(splitmix64(seed) ^ step), m_k = splitmix64(r + k) mod M (uint64),
       C[:,k] = float(x[m_k]), N = 1, S[k] = C[:,k], idle = 0, restarts += 1.
The codebook is held here as C[T, D] (code k = row k); the engine's master is its transpose [D, T].

Error model of the cluster sums (u = 2^-24): an fp32 sum of n terms in ANY order loses at most (n - 1) u sum|x| to first order; the
tests use n u sum|x|, which also covers the second-order terms for n <= 2^20.  Integer-valued x in [-8, 8] with M <= 2^20 keeps every
partial sum an integer below 2^24: those sums are exact in any order."""
import numpy as np

U = 2.0 ** -24
MASK = (1 << 64) - 1

M_VALUES = (1, 7, 1030)          # the sets of tests/vae_vq_ref.py
T_VALUES = (64, 576, 4096)
D_VALUES = (64, 128, 512)
IDX_KINDS = ("uniform", "one_code", "arange", "top8")


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def restart_row(seed, step, k, M):
    """the encoder row that re-seeds code k at this step"""
    r = splitmix64(splitmix64(seed & MASK) ^ (step & MASK))
    return splitmix64((r + k) & MASK) % M


def round_bf16(x):
    """fp32 array -> the nearest bf16 value (ties to even), as fp32"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32)


def make_idx(kind, M, T, seed=0):
    g = np.random.default_rng(1000 + seed)
    if kind == "uniform":
        return g.integers(0, T, M).astype(np.int32)
    if kind == "one_code":
        return np.full(M, T // 2 + 1, np.int32)
    if kind == "arange":
        return (np.arange(M) % T).astype(np.int32)
    if kind == "top8":
        return (T - 8 + g.integers(0, 8, M)).astype(np.int32)
    raise KeyError(kind)


def make_x(M, D, integer, seed=0):
    """bf16-valued fp32 [M, D]: integers in [-8, 8], or standard normals rounded to bf16"""
    g = np.random.default_rng(2000 + seed)
    if integer:
        return g.integers(-8, 9, (M, D)).astype(np.float32)
    return round_bf16(g.standard_normal((M, D)).astype(np.float32))


def cluster_sums64(x, idx, T):
    """counts int64 [T], the float64 sums [T, D] and the sums of magnitudes [T, D]"""
    x64 = np.asarray(x, np.float64)
    n = np.bincount(idx, minlength=T).astype(np.int64)
    s, a = np.zeros((T, x64.shape[1])), np.zeros((T, x64.shape[1]))
    np.add.at(s, idx, x64)
    np.add.at(a, idx, np.abs(x64))
    return n, s, a


def initial_state(C):
    """C fp32 [T, D] -> dict(N, S, idle, restarts)"""
    C = np.asarray(C, np.float32)
    return dict(N=np.ones(C.shape[0], np.float32), S=C.copy(), idle=np.zeros(C.shape[0], np.int32), restarts=0)


def ema_step(C, state, s, n, x, gamma, R=0, seed=0, step=0):
    """one update: returns (C', state', changed) without touching its inputs.  C fp32 [T, D], s fp32 [T, D] and n int [T] the step's
    cluster sums, x fp32 [M, D].  changed[k]: C[k] was rewritten (n[k] > 0 or restarted)."""
    f = np.float32
    g, w = f(gamma), f(1.0 - float(gamma))
    C = np.array(C, np.float32)
    N, S = np.array(state["N"], np.float32), np.array(state["S"], np.float32)
    idle, restarts = np.array(state["idle"], np.int32), int(state["restarts"])
    s, n = np.asarray(s, np.float32), np.asarray(n)
    M, T = x.shape[0], C.shape[0]
    hit = n > 0
    N = (g * N).astype(f)
    S = (g * S).astype(f)
    N[hit] = (N[hit] + (w * n[hit].astype(f)).astype(f)).astype(f)
    S[hit] = (S[hit] + (w * s[hit]).astype(f)).astype(f)
    C[hit] = (S[hit] / N[hit][:, None]).astype(f)
    idle = np.where(hit, 0, idle + 1).astype(np.int32)
    changed = hit.copy()
    if R > 0:
        for k in np.nonzero(idle >= R)[0]:
            row = np.asarray(x[restart_row(seed, step, int(k), M)], np.float32)
            C[k], S[k], N[k], idle[k] = row, row, f(1.0), 0
            restarts += 1
            changed[k] = True
    return C, dict(N=N, S=S, idle=idle, restarts=restarts), changed


def ulp32(v):
    v = np.abs(np.asarray(v, np.float32))
    return np.spacing(np.maximum(v, np.float32(2.0 ** -126))).astype(np.float64)
