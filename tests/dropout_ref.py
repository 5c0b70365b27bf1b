"""numpy restatement of the stateless dropout mask (include/dalle_hip.h "Dropout"; written from the definition, not from
dalle_mtf.dropout); engine_masks gives the per-site masks that the fp32 step oracle (tests/dalle_step_ref.py, dropout=) injects."""
import numpy as np

U = np.uint64


def splitmix64(x):
    """uint64 array (or scalar) -> uint64, wrapping arithmetic"""
    with np.errstate(over="ignore"):
        x = np.asarray(x, dtype=U) + U(0x9E3779B97F4A7C15)
        x = (x ^ (x >> U(30))) * U(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> U(27))) * U(0x94D049BB133111EB)
        return x ^ (x >> U(31))


def site_key(seed, step, microbatch, rank, site):
    k = splitmix64(U(seed))
    k = splitmix64(k ^ U(step))
    k = splitmix64(k ^ U((microbatch << 32) | rank))
    return int(splitmix64(k ^ U(site)))


def threshold(rate):
    return int(min(max(np.rint(rate * 65536.0), 0), 65535))


def scale(thresh):
    return np.float32(65536.0 / (65536 - thresh))


def keep(key, thresh, n):
    """bool [n]: element e of a site's tensor (row-major) is kept"""
    e = np.arange(n, dtype=U)
    with np.errstate(over="ignore"):
        h = splitmix64(U(key) + (e >> U(2)))
    r = (h >> (U(16) * (e & U(3)))) & U(0xffff)
    return r >= U(thresh)


def mask(key, thresh, shape):
    """float32 array of `shape`: scale where kept, 0 where dropped"""
    n = int(np.prod(shape))
    return np.where(keep(key, thresh, n), scale(thresh), np.float32(0)).astype(np.float32).reshape(shape)


def drop(x32, key, thresh):
    """float32 array -> kept ? x * scale : +0 (one fp32 product)"""
    x32 = np.asarray(x32, np.float32)
    k = keep(key, thresh, x32.size).reshape(x32.shape)
    return np.where(k, x32 * scale(thresh), np.float32(0)).astype(np.float32)


def engine_masks(last_dropout, B, S, d, n_layers):
    """{site: float32 mask} from DalleEngine.last_dropout = {site: (key, thresh)}; a site that is absent is all ones"""
    out = {}
    for site in range(2 + 2 * n_layers):
        shape = (S, d) if site == 1 else (B, S, d)
        out[site] = mask(*last_dropout[site], shape) if site in last_dropout else np.ones(shape, np.float32)
    return out
