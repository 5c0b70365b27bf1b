"""float64 restatements of the pointwise and re-layout kernels of the discrete-VAE path (dalle-mtf_amd/csrc/vae.hip): Gumbel-softmax
forward and backward, the MSE loss and its gradient, channel padding, the pixel interleave of the transposed convolution and the
weight gathers.  CPU only (numpy); each function takes the SAME fp32 / bf16-valued inputs the kernel reads, so that a comparison
measures the kernel's arithmetic alone."""
import numpy as np

WG_ROW = 23        # int64 fields per weight_gather_batch table row: in_off, out_off, A, Bn, nsel, ldo, first_block, idx[16]
WG_BLOCK = 2048    # output elements per weight_gather_batch block


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def gumbel_noise(u):
    """g = -log(-log u)"""
    return -np.log(-np.log(_f64(u)))


def gumbel_z(logits, u, temperature):
    """z = (l + g) / T, T the fp32 temperature the kernel is given"""
    return (_f64(logits) + gumbel_noise(u)) / float(np.float32(temperature))


def softmax(z):
    z = _f64(z)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def gumbel_fwd(logits, u, temperature, hard):
    """-> (y, y_soft, index): y_soft = softmax(z); index = first argmax of z (np.argmax, like tf.argmax / torch.argmax, returns the
    lowest of tied indices); y = one-hot(index) when hard, else y_soft"""
    z = gumbel_z(logits, u, temperature)
    p = softmax(z)
    idx = np.argmax(z, axis=-1)
    if not hard:
        return p, p, idx
    y = np.zeros_like(p)
    y[np.arange(p.shape[0]), idx] = 1.0
    return y, p, idx


def top2_gap(z):
    """per row: (index of the max, z_max - z_second)"""
    z = _f64(z)
    part = np.partition(z, z.shape[-1] - 2, axis=-1)[:, -2:]
    return np.argmax(z, axis=-1), part[:, 1] - part[:, 0]


def gumbel_bwd(dy, y_soft, temperature):
    """dlogits = (1/T) * p * (dy - sum_j dy_j p_j)   (straight-through: the same formula in hard mode)"""
    dy, p = _f64(dy), _f64(y_soft)
    dot = (dy * p).sum(axis=-1, keepdims=True)
    return p * (dy - dot) / float(np.float32(temperature))


def mse(img, out, Cin, grad_scale=1.0):
    """img [N, Cin] fp32, out [N, Cp] bf16 values -> (loss = mean((out - img)^2) over N*Cin, dout [N, Cp] =
    2 (out - img) grad_scale / (N*Cin) with 0 on the pad channels)"""
    img, out = _f64(img), _f64(out)
    N = img.shape[0]
    d = out[:, :Cin] - img
    dout = np.zeros_like(out)
    dout[:, :Cin] = 2.0 * d * float(np.float32(grad_scale)) / (N * Cin)
    return float((d * d).sum() / (N * Cin)), dout


def pad_channels(x, Cp):
    """[N, Cin] -> [N, Cp], channels [Cin, Cp) zero (the bf16 rounding is the caller's: torch .to(bfloat16))"""
    x = np.asarray(x)
    out = np.zeros((x.shape[0], Cp), x.dtype)
    out[:, :x.shape[1]] = x
    return out


def unpad_channels(x, Cin):
    return np.ascontiguousarray(np.asarray(x)[:, :Cin])


def pixel_interleave(in4):
    """in4 [4, B, Ht, Wt, C] (output-parity classes p = 2 py + px) -> out [B, 2 Ht, 2 Wt, C], out[b, 2t+py, 2u+px] = in4[p][b, t, u]"""
    in4 = np.asarray(in4)
    _, B, Ht, Wt, C = in4.shape
    out = np.empty((B, 2 * Ht, 2 * Wt, C), in4.dtype)
    for p in range(4):
        py, px = p >> 1, p & 1
        out[:, py::2, px::2, :] = in4[p]
    return out


def weight_gather(inp, idx, ldo):
    """inp [K, A, Bn] -> out [A, ldo], out[a, t*Bn + b] = inp[idx[t], a, b]; columns [len(idx)*Bn, ldo) zero"""
    inp = np.asarray(inp)
    _, A, Bn = inp.shape
    out = np.zeros((A, ldo), inp.dtype)
    for t, k in enumerate(idx):
        out[:, t * Bn:(t + 1) * Bn] = inp[k]
    return out


def gather_table(items):
    """items: [(in_off, out_off, A, Bn, idx, ldo)] -> int64 table [n, WG_ROW]; item i covers output blocks
    [first_block_i, first_block_i + ceil(A*ldo / 2048)) (vae.hip weight_gather_batch).  Returns (table, total blocks)."""
    rows, blk = [], 0
    for in_off, out_off, A, Bn, idx, ldo in items:
        rows.append([in_off, out_off, A, Bn, len(idx), ldo, blk] + list(idx) + [0] * (16 - len(idx)))
        blk += (A * ldo + WG_BLOCK - 1) // WG_BLOCK
    return np.asarray(rows, np.int64), blk


def weight_gather_batch(in_base, out_base, table):
    """every table row applied as one weight_gather of in_base[in_off:] ([K, A, Bn]) into out_base[out_off : out_off + A*ldo];
    the rest of out_base is left as it was"""
    in_base, out = np.asarray(in_base), np.array(out_base, copy=True)
    for r in np.asarray(table, np.int64):
        in_off, out_off, A, Bn, nsel, ldo = (int(v) for v in r[:6])
        idx = [int(v) for v in r[7:7 + nsel]]
        K = max(idx) + 1
        src = in_base[in_off:in_off + K * A * Bn].reshape(K, A, Bn)
        out[out_off:out_off + A * ldo] = weight_gather(src, idx, ldo).reshape(-1)
    return out
