"""ctypes binding of libdalle_hip.so (include/dalle_hip.h).

Thin plumbing only: torch tensors supply device memory and the current HIP stream; every
function below forwards raw pointers + sizes to the C ABI and raises on a non-zero status.
There is NO CPU fallback: if the library is missing or a GPU is absent the call fails loudly.
"""
from __future__ import annotations

import ctypes
import os
import struct

import numpy as np
from ctypes import c_int, c_void_p

import torch

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DALLE_HIP_LIB") or os.path.join(_HERE, "libdalle_hip.so")  # override: A/B of two builds
HEADER_PATH = abi.HEADER_PATH

# signatures, struct fields and constants all come from the header (abi.py): nothing below restates them
_H = abi.header()
GEMM_BIAS, GEMM_RELU, GEMM_RESIDUAL, GEMM_RELU_MASK, GEMM_OUT_F32, GEMM_ROWSCALE, GEMM_GELU = (
    _H.constants["DMI_GEMM_" + n] for n in ("BIAS", "RELU", "RESIDUAL", "RELU_MASK", "OUT_F32", "ROWSCALE", "GELU"))

_lib = None


class DalleHipError(RuntimeError):
    pass


def declared_symbols():
    """Every dmi_* function the public header declares."""
    return sorted(_H.functions)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DalleHipError(
                f"{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc --offload-arch=gfx950). "
                "There is no CPU fallback for the product path.")
        _lib = ctypes.CDLL(LIB_PATH)
        abi.declare(_lib)
        for kv in os.environ.get("DALLE_HIP_OPTIONS", "").split(","):   # A/B hook: e.g. DALLE_HIP_OPTIONS=tn8=0,attn_xcd=0
            if "=" in kv:
                if _lib.dmi_set_option(kv.split("=")[0].strip().encode(), int(kv.split("=")[1])) != 0:
                    raise DalleHipError(f"DALLE_HIP_OPTIONS: unknown option {kv!r}")
    return _lib


def _check(rc, what):
    if rc != 0:
        raise DalleHipError(f"{what}: status {rc}: {lib().dmi_last_error_string().decode()}")


def _p(t):
    """device pointer of a tensor, or a raw device address (int) for sub-buffer views (row chunks)."""
    if t is None:
        return 0
    return t if isinstance(t, int) else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(*ts):
    for t in ts:
        if t is not None and not isinstance(t, int) and not t.is_cuda:
            raise DalleHipError("dalle_hip ops need CUDA(HIP) tensors; there is no CPU fallback")


def set_option(name: str, value: int):
    _check(lib().dmi_set_option(name.encode(), int(value)), "set_option")


def get_option(name: str) -> int:
    return lib().dmi_get_option(name.encode())


# ------------------------------------------------------------------ wrappers (torch tensors in/out)

def embed_fwd(tokens, wte, wpe, x, S, d, vocab, pos_dev=None):
    _dev(tokens, wte, wpe, x)
    _check(lib().dmi_embed_fwd(_p(tokens), _p(wte), _p(wpe), _p(x), tokens.numel(), S, d, vocab, _p(pos_dev), _stream()), "embed_fwd")


def sort_tokens_workspace_bytes(n):
    return int(lib().dmi_sort_tokens_workspace_bytes(n))


def sort_tokens(tokens, sorted_tokens, perm, n, vocab, ws):
    """stable sort of the token ids: sorted_tokens ascending, perm = source positions (int32 device tensors)."""
    _dev(tokens, sorted_tokens, perm, ws)
    _check(lib().dmi_sort_tokens(_p(tokens), _p(sorted_tokens), _p(perm), n, vocab, _p(ws), _stream()), "sort_tokens")


def embed_bwd_workspace_bytes(B, S, d):
    return int(lib().dmi_embed_bwd_workspace_bytes(B, S, d))


def embed_bwd(sorted_tokens, perm, dx, dwte, dwpe, B, S, d, vocab, ws):
    _dev(sorted_tokens, perm, dx, dwte, dwpe, ws)
    _check(lib().dmi_embed_bwd(_p(sorted_tokens), _p(perm), _p(dx), _p(dwte), _p(dwpe), B, S, d, vocab, _p(ws), _stream()),
           "embed_bwd")


def layernorm_fwd(x, g, b, y, mean, rstd, rows, d, eps=1e-5):
    _dev(x, g, b, y, mean, rstd)
    _check(lib().dmi_layernorm_fwd(_p(x), _p(g), _p(b), _p(y), _p(mean), _p(rstd), rows, d, eps, _stream()), "layernorm_fwd")


def embed_fwd_dropout(tokens, wte, wpe, x, S, d, vocab, key_tok, key_pos, thresh):
    """embed_fwd with the token mask (key_tok) and the positional mask (key_pos, shared over the batch) of one threshold"""
    _dev(tokens, wte, wpe, x)
    _check(lib().dmi_embed_fwd_dropout(_p(tokens), _p(wte), _p(wpe), _p(x), tokens.numel(), S, d, vocab, int(key_tok), int(key_pos),
                                       int(thresh), _stream()), "embed_fwd_dropout")


def embed_bwd_dropout(sorted_tokens, perm, dx, dwte, dwpe, B, S, d, vocab, ws, key_tok, key_pos, thresh):
    _dev(sorted_tokens, perm, dx, dwte, dwpe, ws)
    _check(lib().dmi_embed_bwd_dropout(_p(sorted_tokens), _p(perm), _p(dx), _p(dwte), _p(dwpe), B, S, d, vocab, _p(ws), int(key_tok),
                                       int(key_pos), int(thresh), _stream()), "embed_bwd_dropout")


def dropout_add_ln(a, residual, x_out, gamma, beta, y, mean, rstd, M, d, key, thresh, eps=1e-5):
    """x_out = bf16(residual + drop(a)) and, in the same pass, y / mean / rstd = layernorm_fwd(x_out); gamma None: x_out only"""
    _dev(a, residual, x_out, gamma, beta, y, mean, rstd)
    for t in (a, residual, x_out):
        assert t.dtype == torch.bfloat16 and t.numel() >= M * d
    if gamma is not None:
        assert y.dtype == torch.bfloat16 and y.numel() >= M * d and mean.dtype == torch.float32 and rstd.dtype == torch.float32
        assert mean.numel() >= M and rstd.numel() >= M and gamma.numel() >= d and beta.numel() >= d
    _check(lib().dmi_dropout_add_ln(_p(a), _p(residual), _p(x_out), _p(gamma), _p(beta), _p(y), _p(mean), _p(rstd), M, d, int(key),
                                    int(thresh), float(eps), _stream()), "dropout_add_ln")


def dropout_bwd(dx, dy, M, d, key, thresh):
    """dy = bf16(drop(dx)): the gradient of a dropped branch output"""
    _dev(dx, dy)
    assert dx.dtype == torch.bfloat16 and dy.dtype == torch.bfloat16 and dx.numel() >= M * d and dy.numel() >= M * d
    _check(lib().dmi_dropout_bwd(_p(dx), _p(dy), M, d, int(key), int(thresh), _stream()), "dropout_bwd")


def rope_qk(qkv, cs, rows, S, H, head_dim, inverse=False, ld=None):
    """rotates q | k of every row of the [rows, ld] bf16 buffer in the qkv layout in place (ld defaults to 3 H head_dim); row r
    takes row r % S of the (cos, sin) table cs, fp32 [S, head_dim / 2, 2]; inverse: the transpose (the gradient's rotation)"""
    _dev(qkv, cs)
    ld = 3 * H * head_dim if ld is None else int(ld)
    assert qkv.dtype == torch.bfloat16 and qkv.numel() >= rows * ld and cs.dtype == torch.float32 and cs.numel() >= S * head_dim
    _check(lib().dmi_rope_qk(_p(qkv), ld, _p(cs), rows, S, H, head_dim, int(bool(inverse)), _stream()), "rope_qk")


def rope_qk_decode(fresh, cs, B, S, H, head_dim, pos=0, pos_dev=None):
    """rope_qk of the decode step's [B, 3 H head_dim] staging buffer, every row at position pos (pos_dev: read from device memory;
    outside [0, S) the launch writes nothing)"""
    _dev(fresh, cs, pos_dev)
    assert fresh.dtype == torch.bfloat16 and fresh.numel() >= B * 3 * H * head_dim
    assert cs.dtype == torch.float32 and cs.numel() >= S * head_dim and (pos_dev is None or pos_dev.dtype == torch.int32)
    _check(lib().dmi_rope_qk_decode(_p(fresh), _p(cs), B, S, H, head_dim, int(pos), _p(pos_dev), _stream()), "rope_qk_decode")


def qk_norm_fwd(qkv, gq, gk, rows, S, H, head_dim, pre=None, cs=None, ld=None):
    """RMS-normalises q | k of every row of the [rows, ld] bf16 buffer in the qkv layout in place, per head, with the bf16 [head_dim]
    gains gq, gk and head_dim^(-1/2) on q (ld defaults to 3 H head_dim).  pre: also takes the unnormalised q | k, packed bf16
    [rows, 2 H head_dim]; cs: the rope_qk table, whose rotation of row r % S follows in the same pass (one rounding)"""
    _dev(qkv, gq, gk, pre, cs)
    ld = 3 * H * head_dim if ld is None else int(ld)
    assert qkv.dtype == torch.bfloat16 and qkv.numel() >= rows * ld
    assert gq.dtype == torch.bfloat16 and gk.dtype == torch.bfloat16 and gq.numel() >= head_dim and gk.numel() >= head_dim
    assert pre is None or (pre.dtype == torch.bfloat16 and pre.numel() >= rows * 2 * H * head_dim)
    assert cs is None or (cs.dtype == torch.float32 and cs.numel() >= S * head_dim)
    _check(lib().dmi_qk_norm_fwd(_p(qkv), ld, _p(pre), _p(gq), _p(gk), _p(cs), rows, S, H, head_dim, _stream()), "qk_norm_fwd")


def qk_norm_bwd_workspace_bytes(rows, head_dim):
    return int(lib().dmi_qk_norm_bwd_workspace_bytes(rows, head_dim))


def qk_norm_bwd(dqkv, pre, gq, gk, dgq, dgk, ws, rows, S, H, head_dim, cs=None, ld=None):
    """the gradient of qk_norm_fwd, in place on q | k of dqkv (with cs: rotated back first); pre: what the forward kept; dgq, dgk:
    fp32 [head_dim], written; ws: qk_norm_bwd_workspace_bytes(rows, head_dim) bytes"""
    _dev(dqkv, pre, gq, gk, dgq, dgk, ws, cs)
    ld = 3 * H * head_dim if ld is None else int(ld)
    assert dqkv.dtype == torch.bfloat16 and dqkv.numel() >= rows * ld
    assert pre.dtype == torch.bfloat16 and pre.numel() >= rows * 2 * H * head_dim
    assert gq.dtype == torch.bfloat16 and gk.dtype == torch.bfloat16 and gq.numel() >= head_dim and gk.numel() >= head_dim
    assert dgq.dtype == torch.float32 and dgk.dtype == torch.float32 and dgq.numel() >= head_dim and dgk.numel() >= head_dim
    assert ws.numel() * ws.element_size() >= qk_norm_bwd_workspace_bytes(rows, head_dim)
    assert cs is None or (cs.dtype == torch.float32 and cs.numel() >= S * head_dim)
    _check(lib().dmi_qk_norm_bwd(_p(dqkv), ld, _p(pre), _p(gq), _p(gk), _p(cs), _p(dgq), _p(dgk), _p(ws), rows, S, H, head_dim,
                                 _stream()), "qk_norm_bwd")


def qk_norm_decode(fresh, gq, gk, B, S, H, head_dim, cs=None, pos=0, pos_dev=None):
    """qk_norm_fwd of the decode step's [B, 3 H head_dim] staging buffer; with cs every row at position pos (pos_dev: read from
    device memory; outside [0, S) the launch writes nothing), without it the position is not used"""
    _dev(fresh, gq, gk, cs, pos_dev)
    assert fresh.dtype == torch.bfloat16 and fresh.numel() >= B * 3 * H * head_dim
    assert gq.dtype == torch.bfloat16 and gk.dtype == torch.bfloat16 and gq.numel() >= head_dim and gk.numel() >= head_dim
    assert cs is None or (cs.dtype == torch.float32 and cs.numel() >= S * head_dim)
    assert pos_dev is None or pos_dev.dtype == torch.int32
    _check(lib().dmi_qk_norm_decode(_p(fresh), _p(gq), _p(gk), _p(cs), B, S, H, head_dim, int(pos), _p(pos_dev), _stream()),
           "qk_norm_decode")


def token_shift(x, y, rows, S, T, G, d, inverse=False, hist=None):
    """y = shift(x) over dense [rows, d] bf16 buffers (rows a multiple of S = T + G * G): channels [0, d/4) from the previous
    position (image tokens: from the row above), [d/4, d/2) from the previous position (image tokens: from the left), the rest
    unchanged; inverse: the transpose.  hist (forward only): also takes columns [0, d/2) of every input row, bf16 [rows, d/2]"""
    _dev(x, y, hist)
    assert x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and x.numel() >= rows * d and y.numel() >= rows * d
    assert hist is None or (hist.dtype == torch.bfloat16 and hist.numel() >= rows * (d // 2))
    _check(lib().dmi_token_shift(_p(x), _p(y), _p(hist), rows, S, T, G, d, int(bool(inverse)), _stream()), "token_shift")


def token_shift_decode(x, hist, y, B, S, T, G, d, pos=0, pos_dev=None):
    """token_shift of the decode step's [B, d] row at position pos (pos_dev: read from device memory; outside [0, S) the launch
    writes nothing): the neighbours' halves come from hist, bf16 [B, S, d/2], whose row pos then takes x[:, :d/2]"""
    _dev(x, hist, y, pos_dev)
    assert x.dtype == torch.bfloat16 and y.dtype == torch.bfloat16 and x.numel() >= B * d and y.numel() >= B * d
    assert hist.dtype == torch.bfloat16 and hist.numel() >= B * S * (d // 2) and (pos_dev is None or pos_dev.dtype == torch.int32)
    _check(lib().dmi_token_shift_decode(_p(x), _p(hist), _p(y), B, S, T, G, d, int(pos), _p(pos_dev), _stream()), "token_shift_decode")


def layernorm_bwd_workspace_bytes(rows, d):
    return lib().dmi_layernorm_bwd_workspace_bytes(rows, d)


def layernorm_bwd(dy, x, g, mean, rstd, dres, dx, dg, db, ws, rows, d):
    """dg = db = None: deferred -- the partials stay in `ws` until layernorm_bwd_finish_batch"""
    _dev(dy, x, g, mean, rstd, dx, ws)
    _check(lib().dmi_layernorm_bwd(_p(dy), _p(x), _p(g), _p(mean), _p(rstd), _p(dres), _p(dx), _p(dg), _p(db),
                                   _p(ws), rows, d, _stream()), "layernorm_bwd")


def layernorm_bwd_finish_batch(items, d):
    """items: [(workspace, dg, db, rows)] of deferred layernorm_bwd calls (at most 16, one width)"""
    import ctypes
    n = len(items)
    PA, LA = ctypes.c_void_p * n, ctypes.c_int64 * n
    _check(lib().dmi_layernorm_bwd_finish_batch(PA(*[_p(i[0]) for i in items]), PA(*[_p(i[1]) for i in items]), PA(*[_p(i[2]) for i in items]),
                                                LA(*[int(i[3]) for i in items]), n, d, _stream()), "layernorm_bwd_finish_batch")


def gemm_nt(A, lda, Bt, ldb, C, ldc, M, N, K, flags=0, bias=None, residual=None, relu_src=None, rowscale=None):
    _dev(A, Bt, C)
    _check(lib().dmi_gemm_nt(_p(A), lda, _p(Bt), ldb, _p(C), ldc, M, N, K, flags, _p(bias), _p(residual),
                             _p(relu_src), _p(rowscale), _stream()), "gemm_nt")


def gemm_nt_ln(A, lda, Bt, ldb, C, ldc, M, N, K, gamma, beta, Y, ldy, mean, rstd, bias=None, residual=None, eps=1e-5):
    """C = bf16(A . Bt^T + bias + residual) and, in the same pass, Y = LayerNorm(C) * gamma + beta with the row statistics
    (N = 512: full-row tiles).  Raises DalleHipError (unsupported) for other widths: the caller keeps gemm_nt + layernorm_fwd."""
    _dev(A, Bt, C, gamma, beta, Y, mean, rstd)
    assert mean.dtype == torch.float32 and rstd.dtype == torch.float32 and mean.numel() >= M and rstd.numel() >= M
    _check(lib().dmi_gemm_nt_ln(_p(A), lda, _p(Bt), ldb, _p(C), ldc, M, N, K, _p(bias), _p(residual), _p(gamma), _p(beta), float(eps),
                                _p(Y), ldy, _p(mean), _p(rstd), _stream()), "gemm_nt_ln")


def gemm_nt_lnbwd_parts(M):
    return int(lib().dmi_gemm_nt_lnbwd_parts(M))


def gemm_nt_lnbwd(A, lda, Bt, ldb, M, N, K, x, gamma, mean, rstd, dres, dx, part, dg=None, db=None, B2=None, ldb2=0, C2=None):
    """dx = LayerNorm-backward(x; gamma, mean, rstd)(A . Bt^T) + dres in one pass (N = 512: full-row tiles); part: fp32
    [gemm_nt_lnbwd_parts(M), 2 N] partial gain | bias gradients.  dg / db given: the partials are summed into them right away.
    B2 / C2: the product that consumes dx chained in the same launch, C2 = dx . B2^T."""
    _dev(A, Bt, x, gamma, mean, rstd, dres, dx, part, dg, db, B2, C2)
    P = gemm_nt_lnbwd_parts(M)
    assert part.dtype == torch.float32 and part.numel() >= P * 2 * N
    _check(lib().dmi_gemm_nt_lnbwd(_p(A), lda, _p(Bt), ldb, M, N, K, _p(x), _p(gamma), _p(mean), _p(rstd), _p(dres), _p(dx), _p(part),
                                   _p(B2), ldb2, _p(C2), _stream()), "gemm_nt_lnbwd")
    if dg is not None:
        _check(lib().dmi_layernorm_bwd_finish_parts(_p(part), P, _p(dg), _p(db), N, _stream()), "layernorm_bwd_finish_parts")


def relu_bits_bytes(M, N):
    return int(lib().dmi_relu_bits_bytes(M, N))


def gemm_nt_ln_auto(M, N, K):
    """True where gemm_nt_ln / gemm_nt_lnbwd accept the shape and the library would pick the full-row kernel itself."""
    return bool(lib().dmi_gemm_nt_ln_auto(M, N, K))


def relu_bits_auto(M, N, K):
    """True where the library's dispatch runs [M, N, K] on the kernel that has the bit forms of the ReLU mask"""
    return bool(lib().dmi_relu_bits_auto(M, N, K))


def gemm_nt_relu_bits(A, lda, Bt, ldb, C, ldc, M, N, K, bias, bits):
    """C = bf16(relu(A . Bt^T + bias)); bits (uint8, relu_bits_bytes(M, N)) = one bit per output, C > 0"""
    _dev(A, Bt, C, bias, bits)
    assert bits.dtype == torch.uint8 and bits.numel() >= relu_bits_bytes(M, N)
    _check(lib().dmi_gemm_nt_relu_bits(_p(A), lda, _p(Bt), ldb, _p(C), ldc, M, N, K, _p(bias), _p(bits), _stream()), "gemm_nt_relu_bits")


def gemm_nt_mask_bits(A, lda, Bt, ldb, C, ldc, M, N, K, bits):
    """C = bf16(A . Bt^T) where the bit written by gemm_nt_relu_bits is set, 0 elsewhere (= gemm_nt with GEMM_RELU_MASK, relu_src = h)"""
    _dev(A, Bt, C, bits)
    assert bits.dtype == torch.uint8 and bits.numel() >= relu_bits_bytes(M, N)
    _check(lib().dmi_gemm_nt_mask_bits(_p(A), lda, _p(Bt), ldb, _p(C), ldc, M, N, K, _p(bits), _stream()), "gemm_nt_mask_bits")


def gemm_nt_gelu(A, lda, Bt, ldb, C, ldc, M, N, K, bias, pre, ldpre):
    """a = A . Bt^T + bias (fp32): C = bf16(gelu(a)) (tanh form) and pre = bf16(a) [M, ldpre], the input of gemm_nt_gelu_grad"""
    _dev(A, Bt, C, bias, pre)
    _check(lib().dmi_gemm_nt_gelu(_p(A), lda, _p(Bt), ldb, _p(C), ldc, M, N, K, _p(bias), _p(pre), ldpre, _stream()), "gemm_nt_gelu")


def gemm_nt_gelu_grad(A, lda, Bt, ldb, C, ldc, M, N, K, pre, ldpre):
    """C = bf16((A . Bt^T) * gelu'(pre)), pre as gemm_nt_gelu wrote it"""
    _dev(A, Bt, C, pre)
    _check(lib().dmi_gemm_nt_gelu_grad(_p(A), lda, _p(Bt), ldb, _p(C), ldc, M, N, K, _p(pre), ldpre, _stream()), "gemm_nt_gelu_grad")


def _glu_act(act):
    if act not in ("relu", "gelu"):
        raise DalleHipError(f"glu: act must be 'relu' or 'gelu' (got {act!r})")
    return GEMM_GELU if act == "gelu" else GEMM_RELU


def _glu_rows(t, ld, M, cols):
    """t holds M rows of `cols` bf16 elements at leading dimension ld (the last row need not be padded)"""
    if not isinstance(t, int):       # (a raw device address is the caller's to size)
        assert t.dtype == torch.bfloat16 and t.numel() >= (M - 1) * ld + cols


def glu_fwd(pre, ldpre, h, ldh, M, Hh, act):
    """h[m, j] = bf16(pre[m, j] * act(pre[m, Hh + j])): the gated FFN's hidden layer from pre = [value | gate]; act "relu" / "gelu" """
    _dev(pre, h)
    _glu_rows(pre, ldpre, M, 2 * Hh)
    _glu_rows(h, ldh, M, Hh)
    _check(lib().dmi_glu_fwd(_p(pre), ldpre, _p(h), ldh, M, Hh, _glu_act(act), _stream()), "glu_fwd")


def glu_bwd(dh, lddh, pre, ldpre, dpre, lddpre, M, Hh, act):
    """dpre[m, j] = bf16(dh * act(gate)), dpre[m, Hh + j] = bf16(dh * val * act'(gate)) from dh [M, Hh] and pre as glu_fwd read it"""
    _dev(dh, pre, dpre)
    _glu_rows(dh, lddh, M, Hh)
    _glu_rows(pre, ldpre, M, 2 * Hh)
    _glu_rows(dpre, lddpre, M, 2 * Hh)
    _check(lib().dmi_glu_bwd(_p(dh), lddh, _p(pre), ldpre, _p(dpre), lddpre, M, Hh, _glu_act(act), _stream()), "glu_bwd")


def ln_gemm_nt(X, ldx, gamma, beta, Bt, ldb, C, ldc, M, N, K, flags=0, bias=None, eps=1e-5):
    """C = LayerNorm(X) . Bt^T (+ bias)(ReLU / GELU) for the decode step (M <= 32)"""
    _dev(X, gamma, beta, Bt, C)
    _check(lib().dmi_ln_gemm_nt(_p(X), ldx, _p(gamma), _p(beta), eps, _p(Bt), ldb, _p(C), ldc, M, N, K, flags, _p(bias), _stream()),
           "ln_gemm_nt")


def attention_decode(qkv, o, B, H, S, pos, fresh=None, pos_dev=None, head_dim=128):
    """one query position against the K/V cache held in the [B*S, 3d] projection buffer.  fresh=None: row pos already
    written; fresh = [B, 3d] staging buffer: the kernel moves it into row pos.  pos_dev (int32 [1] on the device) overrides
    pos -- the graph-replayable form.  head_dim: 64 or 128 (d = H * head_dim)."""
    _dev(qkv, o)
    if fresh is not None:
        _dev(fresh)
    if pos_dev is not None:
        _dev(pos_dev)
        assert pos_dev.dtype == torch.int32
    _check(lib().dmi_attention_decode_hd(_p(qkv), _p(fresh), _p(o), B, H, S, int(pos), _p(pos_dev), int(head_dim), _stream()),
           "attention_decode")


def _kv8_check(data, scale, B, S, H, head_dim):
    _dev(data, scale)
    assert data.dtype == torch.uint8 and data.numel() >= B * S * 2 * H * head_dim
    assert scale.dtype == torch.float32 and scale.numel() >= B * S * 2 * H


def kv8_quantize(qkv, data, scale, B, S, H, head_dim, s0, s1, ld=None):
    """rows s0 <= s < s1 of every sequence of the bf16 [B*S, ld] q | k | v buffer (ld defaults to 3 H head_dim) into the FP8 cache:
    data uint8 [B, S, 2, H, head_dim] (E4M3FN) and scale fp32 [B, S, 2, H], one power of two per (position, head)"""
    _dev(qkv)
    _kv8_check(data, scale, B, S, H, head_dim)
    ld = 3 * H * head_dim if ld is None else int(ld)
    assert qkv.dtype == torch.bfloat16 and qkv.numel() >= B * S * ld
    _check(lib().dmi_kv8_quantize(_p(qkv), ld, _p(data), _p(scale), B, S, H, int(head_dim), int(s0), int(s1), _stream()), "kv8_quantize")


def attention_decode_kv8(data, scale, fresh, o, B, H, S, pos, pos_dev=None, head_dim=128, plan=None):
    """attention_decode over the FP8 cache (data, scale) of kv8_quantize: q from the [B, 3d] staging buffer `fresh`, whose k and v
    are quantised into cache row pos; every key and value attended to is a dequantised one.  plan: an AttnMaskPlan (row pos of it)"""
    _dev(fresh, o, pos_dev)
    _kv8_check(data, scale, B, S, H, head_dim)
    assert fresh.dtype == torch.bfloat16 and fresh.numel() >= B * 3 * H * head_dim and (pos_dev is None or pos_dev.dtype == torch.int32)
    if plan is None:
        _check(lib().dmi_attention_decode_kv8(_p(data), _p(scale), _p(fresh), _p(o), B, H, S, int(pos), _p(pos_dev), int(head_dim),
                                              _stream()), "attention_decode_kv8")
    else:
        _check(lib().dmi_attention_decode_kv8_masked(_p(data), _p(scale), _p(fresh), _p(o), _p(plan.dev), plan.host.ctypes.data, B, H, S,
                                                     int(pos), _p(pos_dev), int(head_dim), _stream()), "attention_decode_kv8_masked")


def gemm_nt_splitk_workspace_bytes(M, N, nsplit):
    return lib().dmi_gemm_nt_splitk_workspace_bytes(M, N, nsplit)


def gemm_nt_splitk(A, lda, Bt, ldb, C, M, N, K, nsplit, ws, rowscale=None):
    _dev(A, Bt, C, ws)
    _check(lib().dmi_gemm_nt_splitk(_p(A), lda, _p(Bt), ldb, _p(C), M, N, K, nsplit, _p(rowscale), _p(ws), _stream()),
           "gemm_nt_splitk")


def gemm_tn_workspace_bytes(M, I, J):
    return lib().dmi_gemm_tn_workspace_bytes(M, I, J)


class ReduceItem(ctypes.Structure):
    """dmi_reduce_item (include/dalle_hip.h)."""
    _fields_ = _H.structs["dmi_reduce_item"]


class DeferredReduces:
    """collects the slab reduces that dmi_gemm_tn calls leave behind; run() launches them as one kernel"""

    def __init__(self, capacity=16):
        self.items = (ReduceItem * capacity)()
        self.n, self.capacity = 0, capacity

    def run(self):
        if self.n:
            _check(lib().dmi_reduce_slabs_batch(ctypes.byref(self.items), self.n, _stream()), "reduce_slabs_batch")
        self.n = 0


def gemm_tn(X, ldx, dY, ldy, dW, M, I, J, ws, dbias=None, bias_weights=None, deferred: "DeferredReduces" = None):
    """deferred: the final slab reduces are appended to it instead of being launched (ws must then be exclusive to this call
    until deferred.run())."""
    _dev(X, dY, dW, ws, dbias, bias_weights)
    if deferred is None:
        _check(lib().dmi_gemm_tn(_p(X), ldx, _p(dY), ldy, _p(dW), _p(dbias), _p(bias_weights), M, I, J, _p(ws), None, None,
                                 _stream()), "gemm_tn")
        return
    assert deferred.n + 2 <= deferred.capacity
    cnt = c_int(0)
    slot = ctypes.byref(deferred.items, deferred.n * ctypes.sizeof(ReduceItem))
    _check(lib().dmi_gemm_tn(_p(X), ldx, _p(dY), ldy, _p(dW), _p(dbias), _p(bias_weights), M, I, J, _p(ws), slot,
                             ctypes.byref(cnt), _stream()), "gemm_tn")
    deferred.n += cnt.value


class TnProblem(ctypes.Structure):
    """dmi_tn_problem (include/dalle_hip.h)."""
    _fields_ = _H.structs["dmi_tn_problem"]


def gemm_tn_group_plan(shapes, M):
    """row splits of the grouped launch of weight gradients with shapes [(I, J), ...] when it runs on 128 x 256 tiles, 0 otherwise"""
    n = len(shapes)
    Is, Js = (c_int * n)(*[s[0] for s in shapes]), (c_int * n)(*[s[1] for s in shapes])
    return int(lib().dmi_gemm_tn_group_plan(Is, Js, n, M))


def gemm_tn_group(problems, M, deferred: "DeferredReduces" = None):
    """several weight gradients over the same M rows in one launch.  problems: dicts with X, ldx, dY, ldy, dW, I, J, ws and
    optionally dbias, bias_weights (as gemm_tn); deferred as in gemm_tn."""
    n = len(problems)
    arr = (TnProblem * n)()
    for k, q in enumerate(problems):
        _dev(q["X"], q["dY"], q["dW"], q["ws"], q.get("dbias"), q.get("bias_weights"))
        assert q["ws"].numel() * q["ws"].element_size() >= gemm_tn_workspace_bytes(M, q["I"], q["J"])
        arr[k] = TnProblem(_p(q["X"]), q["ldx"], _p(q["dY"]), q["ldy"], _p(q["dW"]), _p(q.get("dbias")), _p(q.get("bias_weights")),
                           q["I"], q["J"], _p(q["ws"]))
    if deferred is None:
        _check(lib().dmi_gemm_tn_group(ctypes.byref(arr), n, M, None, None, _stream()), "gemm_tn_group")
        return
    assert deferred.n + 2 * n <= deferred.capacity
    cnt = c_int(0)
    slot = ctypes.byref(deferred.items, deferred.n * ctypes.sizeof(ReduceItem))
    _check(lib().dmi_gemm_tn_group(ctypes.byref(arr), n, M, slot, ctypes.byref(cnt), _stream()), "gemm_tn_group")
    deferred.n += cnt.value


def colsum_workspace_bytes(M, N):
    return lib().dmi_colsum_workspace_bytes(M, N)


def colsum(Y, ldy, out, M, N, ws):
    _dev(Y, out, ws)
    _check(lib().dmi_colsum(_p(Y), ldy, _p(out), M, N, _p(ws), _stream()), "colsum")


def transpose(inp, out, batch, R, C):
    _dev(inp, out)
    _check(lib().dmi_transpose_bf16(_p(inp), _p(out), batch, R, C, _stream()), "transpose")


def set_debug_buffer(t):
    """tools only: u64 device tensor [blocks, 5] receiving per-block phase timestamps of the 256x128 NT kernel (None: off)."""
    lib().dmi_set_debug_buffer(_p(t))


def transpose_batch(in_base, out_base, table, n, total_tiles):
    """table: int64 device tensor [n,5] = {in_off, out_off, R, C, first_tile}."""
    _dev(in_base, out_base, table)
    _check(lib().dmi_transpose_bf16_batch(_p(in_base), _p(out_base), _p(table), n, total_tiles, _stream()), "transpose_batch")


def attention_fwd(qkv, o, lse, B, H, S, head_dim=128):
    """causal attention over qkv [B*S, 3*H*head_dim]; head_dim: 64 or 128"""
    _dev(qkv, o, lse)
    _check(lib().dmi_attention_fwd_hd(_p(qkv), _p(o), _p(lse), B, H, S, int(head_dim), _stream()), "attention_fwd")


def attention_bwd(qkv, o, d_o, lse, scratch, dqkv, B, H, S, head_dim=128):
    _dev(qkv, o, d_o, lse, scratch, dqkv)
    _check(lib().dmi_attention_bwd_hd(_p(qkv), _p(o), _p(d_o), _p(lse), _p(scratch), _p(dqkv), B, H, S, int(head_dim), _stream()),
           "attention_bwd")


# header words of a mask plan (the AMP_* enum of csrc/attention.hip; word 0 is the magic)
PLAN_MAGIC = 0x504D4144
PLAN_HDR = dict(S=1, NB=2, W=3, CAUSAL=4, FPTR=5, FLIST=6, KPTR=7, KLIST=8, FORDER=9, KORDER=10, ROWBITS=11, COLBITS=12, WORDS=13,
                LIVE_F=14, CAUSAL_F=15, LIVE_K=16, CAUSAL_K=17)


class AttnMaskPlan:
    """a compiled attention mask (dmi_attn_mask_plan): `host` int32 numpy words, `dev` the same words on the device.
    mask: bool / uint8 [S, S] (True = query i may attend to key j); it must be causal with no empty row."""

    def __init__(self, mask, device="cuda"):
        m = np.ascontiguousarray(np.asarray(mask.cpu() if hasattr(mask, "cpu") else mask).astype(np.uint8))
        if m.ndim != 2 or m.shape[0] != m.shape[1]:
            raise DalleHipError(f"attn_mask_plan: the mask must be [S, S] (got {m.shape})")
        self.S = int(m.shape[0])
        fn = lib().dmi_attn_mask_plan
        nbytes = fn(m.ctypes.data, self.S, None, 0)
        if nbytes < 0:
            _check(int(nbytes), "attn_mask_plan")
        self.host = np.zeros(nbytes // 4, dtype=np.int32)
        _check(0 if fn(m.ctypes.data, self.S, self.host.ctypes.data, nbytes) == nbytes else -1, "attn_mask_plan")
        assert self.host[0] == PLAN_MAGIC and self.host[PLAN_HDR["S"]] == self.S
        self.causal = bool(self.host[PLAN_HDR["CAUSAL"]])
        self.dev = torch.from_numpy(self.host).to(device) if device is not None else None

    def live_fraction(self):
        """live 32-query x 64-key tiles of the forward / dQ kernels, as a fraction of the causal mask's"""
        return float(self.host[PLAN_HDR["LIVE_F"]]) / float(self.host[PLAN_HDR["CAUSAL_F"]])

    def live_fraction_dkv(self):
        """live 32-query x 128-key tiles of the dK/dV kernel, as a fraction of the causal mask's"""
        return float(self.host[PLAN_HDR["LIVE_K"]]) / float(self.host[PLAN_HDR["CAUSAL_K"]])


def attn_mask_plan_bytes(mask_u8, S):
    """size query of dmi_attn_mask_plan (status < 0 on a refused mask)"""
    m = np.ascontiguousarray(mask_u8, dtype=np.uint8)
    return int(lib().dmi_attn_mask_plan(m.ctypes.data, int(S), None, 0))


def attention_fwd_masked(qkv, o, lse, plan, B, H, S, head_dim=128):
    """attention over qkv under a compiled mask (AttnMaskPlan); a causal plan runs attention_fwd's kernels"""
    _dev(qkv, o, lse)
    _check(lib().dmi_attention_fwd_masked(_p(qkv), _p(o), _p(lse), _p(plan.dev), plan.host.ctypes.data, B, H, S, int(head_dim),
                                          _stream()), "attention_fwd_masked")


def attention_bwd_masked(qkv, o, d_o, lse, scratch, dqkv, plan, B, H, S, head_dim=128):
    _dev(qkv, o, d_o, lse, scratch, dqkv)
    _check(lib().dmi_attention_bwd_masked(_p(qkv), _p(o), _p(d_o), _p(lse), _p(scratch), _p(dqkv), _p(plan.dev), plan.host.ctypes.data,
                                          B, H, S, int(head_dim), _stream()), "attention_bwd_masked")


def attention_decode_masked(qkv, o, plan, B, H, S, pos, fresh=None, pos_dev=None, head_dim=128):
    _check(lib().dmi_attention_decode_masked(_p(qkv), _p(fresh), _p(o), _p(plan.dev), plan.host.ctypes.data, B, H, S, int(pos),
                                             _p(pos_dev), int(head_dim), _stream()), "attention_decode_masked")


def shift_labels(tokens, labels, B, S, eos):
    _dev(tokens, labels)
    _check(lib().dmi_shift_labels(_p(tokens), _p(labels), B, S, eos, _stream()), "shift_labels")


def cross_entropy(z, ldz, labels, loss_rows, lse, M, V, dz_scale):
    _dev(z, labels, loss_rows)
    _check(lib().dmi_cross_entropy(_p(z), ldz, _p(labels), _p(loss_rows), _p(lse), M, V, dz_scale, _stream()), "cross_entropy")


def label_logit(X, ldx, Wt, ldw, bias, labels, zl, flag, M, K, V):
    _dev(X, Wt, bias, labels, zl, flag)
    _check(lib().dmi_label_logit(_p(X), ldx, _p(Wt), ldw, _p(bias), _p(labels), _p(zl), _p(flag), M, K, V, _stream()), "label_logit")


def gemm_nt_softmax_partials(N):
    return int(lib().dmi_gemm_nt_softmax_partials(N))


def gemm_nt_softmax(X, ldx, Wt, ldw, bias, rowshift, E, lde, rowsum_part, M, N, K):
    _dev(X, Wt, bias, E, rowsum_part)
    _check(lib().dmi_gemm_nt_softmax(_p(X), ldx, _p(Wt), ldw, _p(bias), _p(rowshift), _p(E), lde, _p(rowsum_part), M, N, K,
                                     _stream()), "gemm_nt_softmax")


def softmax_finish(rowsum_part, nparts, label_logit, rowshift, labels, X, ldx, Wt, ldw, bias, E, lde, N, loss_rows, rowscale,
                   rowscale_bf16, Xs, flag, M, K, V, dz_scale):
    _dev(rowsum_part, label_logit, rowshift, labels, X, Wt, bias, E, loss_rows, flag)
    _check(lib().dmi_softmax_finish(_p(rowsum_part), nparts, _p(label_logit), _p(rowshift), _p(labels), _p(X), ldx, _p(Wt), ldw,
                                    _p(bias), _p(E), lde, N,
                                    _p(loss_rows), _p(rowscale), _p(rowscale_bf16), _p(Xs), _p(flag), M, K, V, float(dz_scale),
                                    _stream()), "softmax_finish")


def softmax_finish_w(rowsum_part, nparts, label_logit, rowshift, labels, X, ldx, Wt, ldw, bias, E, lde, N, loss_rows, rowscale,
                     rowscale_bf16, Xs, flag, M, K, V, dz_scale, pos_weight, period):
    """softmax_finish with the static loss weight pos_weight[m % period] (fp32) in row m's gradient scale"""
    _dev(rowsum_part, label_logit, rowshift, labels, X, Wt, bias, E, loss_rows, flag, pos_weight)
    _check(lib().dmi_softmax_finish_w(_p(rowsum_part), nparts, _p(label_logit), _p(rowshift), _p(labels), _p(X), ldx, _p(Wt), ldw,
                                      _p(bias), _p(E), lde, N,
                                      _p(loss_rows), _p(rowscale), _p(rowscale_bf16), _p(Xs), _p(flag), M, K, V, float(dz_scale),
                                      _p(pos_weight), int(period), _stream()), "softmax_finish_w")


def sum_f32(x, n, scale, out):
    _dev(x, out)
    _check(lib().dmi_sum_f32(_p(x), n, scale, _p(out), _stream()), "sum_f32")


def loss_reduce(loss_rows, n, pos_weight, period, split, scale, out3):
    """out3 fp32 [3] = (scale * sum_m pos_weight[m % period] * loss_rows[m], mean over m % period < split, mean over the rest)"""
    _dev(loss_rows, pos_weight, out3)
    _check(lib().dmi_loss_reduce(_p(loss_rows), n, _p(pos_weight), int(period), int(split), float(scale), _p(out3), _stream()),
           "loss_reduce")


def loss_mask(labels, M, period, split, pad_id, ct, ci, plain, counts, row_w):
    """counts int32 [2] = (kept text rows, image rows), row_w fp32 [M] = every row's loss weight with the text rows whose label is
    pad_id ignored (include/dalle_hip.h); text rows: m % period < split"""
    _dev(labels, counts, row_w)
    _check(lib().dmi_loss_mask(_p(labels), M, int(period), int(split), int(pad_id), float(ct), float(ci), int(bool(plain)), _p(counts),
                               _p(row_w), _stream()), "loss_mask")


def loss_reduce_masked(loss_rows, row_w, labels, M, period, split, pad_id, counts, scale, out4):
    """out4 fp32 [4] = (scale * sum_m row_w[m] * loss_rows[m], mean over the kept text rows, mean over the image rows, kept text rows /
    text rows); counts: loss_mask's"""
    _dev(loss_rows, row_w, labels, counts, out4)
    _check(lib().dmi_loss_reduce_masked(_p(loss_rows), _p(row_w), _p(labels), M, int(period), int(split), int(pad_id), _p(counts),
                                        float(scale), _p(out4), _stream()), "loss_reduce_masked")


def assemble_tokens(text, vae_logits, tokens_out, B, T, P, C, text_vocab):
    _dev(text, vae_logits, tokens_out)
    _check(lib().dmi_assemble_tokens(_p(text), _p(vae_logits), _p(tokens_out), B, T, P, C, text_vocab, _stream()), "assemble_tokens")


def _draw(name, z, ldz, bias, rows, nv, temperature, top_k, seed, extra, pos, token_offset, next_tok, out, out_col0, params_dev,
          pos_dev, advance, logp=None, tok_rows=None):
    """the checks that the three draws share, then dmi_<name>.  extra: the by-value arguments that the entry point takes after
    seed -- () / (top_p,) / (top_p, scale); with any of them the device parameter block has six words.  rows: B, or the Bc pairs
    of the guided draw, whose next_tok holds tok_rows = 2 * Bc"""
    _dev(z)
    assert z.dtype == torch.bfloat16 and (bias is None or bias.dtype == torch.bfloat16)
    if pos_dev is not None:
        assert pos_dev.dtype == torch.int32 and pos_dev.numel() >= (2 if advance else 1), \
            f"{name}: pos_dev must be int32 [2] ([position, zeroed counter]) when advance=True, int32 [1] otherwise"
    if params_dev is not None and extra:
        assert params_dev.numel() >= 6 and params_dev.element_size() == 4, f"{name}: params_dev must be 32-bit [6]"
    if tok_rows is not None:
        if next_tok is not None:
            assert next_tok.dtype == torch.int32 and next_tok.numel() >= tok_rows, f"{name}: next_tok must be int32 [2 * Bc]"
        if out is not None:
            assert out.dtype == torch.int32 and out.dim() == 2 and out.shape[0] >= rows, f"{name}: out must be int32 [Bc, n]"
    if logp is not None:
        assert logp.dtype == torch.float32 and logp.numel() >= rows, f"{name}: logp must be fp32 [{'Bc' if tok_rows else 'B'}]"
    for t in (bias, next_tok, out, params_dev, pos_dev, logp):
        if t is not None:
            _dev(t)
    out_ld = int(out.shape[1]) if out is not None else 0
    tail = (_p(logp),) if extra else ()
    _check(getattr(lib(), "dmi_" + name)(_p(z), ldz, _p(bias), rows, nv, float(temperature), int(top_k), int(seed) & (2 ** 64 - 1),
                                         *map(float, extra), _p(params_dev), int(pos), _p(pos_dev), int(bool(advance)),
                                         int(token_offset), _p(next_tok), _p(out), out_ld, int(out_col0), *tail, _stream()), name)


def sample_tokens(z, ldz, bias, B, nv, temperature=1.0, top_k=0, seed=0, pos=0, token_offset=0, next_tok=None, out=None,
                  out_col0=0, params_dev=None, pos_dev=None, advance=False):
    """next image token per row of head logits z bf16 [B, ldz] (+ bias bf16 [nv]): temperature / top-k / greedy; the draw is
    a pure function of (seed, position, row).  params_dev (uint32 [4]) / pos_dev (int32) override the by-value settings.
    pos_dev is int32 [1] (the position) -- or, with advance=True, int32 [2]: [position, arrival counter]; the kernel's last
    block to finish increments [0] and resets [1], which must be zero on entry (include/dalle_hip.h)."""
    _draw("sample_tokens", z, ldz, bias, B, nv, temperature, top_k, seed, (), pos, token_offset, next_tok, out, out_col0, params_dev,
          pos_dev, advance)


def sample_tokens_p(z, ldz, bias, B, nv, temperature=1.0, top_k=0, seed=0, top_p=1.0, pos=0, token_offset=0, next_tok=None,
                    out=None, out_col0=0, params_dev=None, pos_dev=None, advance=False, logp=None):
    """sample_tokens with a nucleus (top-p) filter after the top-k one, and optionally the row's log-likelihood of the choice:
    logp fp32 [B] (zeroed by the caller) += log_softmax(z + bias)[choice] at temperature 1, unfiltered.  params_dev is uint32 [6]:
    {bits of 1/temperature (0: greedy), top_k, seed lo, seed hi, bits of top_p, 0}.  At top_p = 1 the tokens are sample_tokens'
    bit for bit (include/dalle_hip.h)."""
    _draw("sample_tokens_p", z, ldz, bias, B, nv, temperature, top_k, seed, (top_p,), pos, token_offset, next_tok, out, out_col0,
          params_dev, pos_dev, advance, logp)


def sample_tokens_guided(z, ldz, bias, Bc, nv, temperature=1.0, top_k=0, seed=0, top_p=1.0, scale=1.0, pos=0, token_offset=0,
                         next_tok=None, out=None, out_col0=0, params_dev=None, pos_dev=None, advance=False, logp=None):
    """classifier-free guidance: sample_tokens_p drawn from g = zc + (scale - 1) * (zc - zu), zc / zu rows b / Bc + b of
    z bf16 [2 * Bc, ldz] (+ bias); one token per pair, written to next_tok[b] and next_tok[Bc + b] (int32 [2 * Bc]) and to
    out int32 [Bc, out_ld]; logp fp32 [Bc] += log_softmax(zc)[choice].  params_dev is uint32 [6] with word 5 = bits of scale
    (sample_params(..., guidance_scale=)).  scale = 1 draws sample_tokens_p's tokens of the first Bc rows (include/dalle_hip.h)."""
    _draw("sample_tokens_guided", z, ldz, bias, Bc, nv, temperature, top_k, seed, (top_p, scale), pos, token_offset, next_tok, out,
          out_col0, params_dev, pos_dev, advance, logp, tok_rows=2 * Bc)


def sample_params(temperature=1.0, top_k=0, seed=0, top_p=None, guidance_scale=None):
    """the device parameter block of the draw kernels as int32 (bit pattern of the uint32 words): [4] for sample_tokens,
    [6] for sample_tokens_p when top_p is given; guidance_scale (with top_p) puts the bits of the scale into word 5 for
    sample_tokens_guided -- without it word 5 is 0, as the unguided kernels have always been given"""
    def bits(x):
        return struct.unpack("<I", struct.pack("<f", x))[0]
    words = [bits(1.0 / temperature if temperature > 0 else 0.0), int(top_k), int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff]
    if guidance_scale is not None:
        assert top_p is not None, "sample_params: guidance_scale goes with top_p (the six-word block)"
        words += [bits(top_p), bits(guidance_scale)]
    elif top_p is not None:
        words += [bits(top_p), 0]
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in words], dtype=torch.int32)


def logits_f32(z, ldz, bias, out, B, nv):
    """out fp32 [B, nv] = float(z bf16 [B, ldz][:, :nv]) + float(bias bf16 [nv] or None)"""
    _dev(z, out)
    assert z.dtype == torch.bfloat16 and out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= B * nv
    if bias is not None:
        _dev(bias)
        assert bias.dtype == torch.bfloat16
    _check(lib().dmi_logits_f32(_p(z), int(ldz), _p(bias), _p(out), int(B), int(nv), _stream()), "logits_f32")


def sumsq_workspace_bytes(n):
    return lib().dmi_sumsq_workspace_bytes(n)


def sumsq(g, n, out, ws):
    _dev(g, out, ws)
    _check(lib().dmi_sumsq(_p(g), n, _p(out), _p(ws), _stream()), "sumsq")


def adam_step(p, g, m, v, p_bf16, n, gnorm_sq, clip, lr, beta1, beta2, eps, wd, grad_scale=1.0, lr_dev=None):
    """lr_dev: optional 1-element fp32 DEVICE tensor the kernel reads the learning rate from (HIP-graph replay)"""
    _dev(p, g, m, v)
    _check(lib().dmi_adam_step(_p(p), _p(g), _p(m), _p(v), _p(p_bf16), n, _p(gnorm_sq), clip, lr, beta1, beta2, eps,
                               wd, grad_scale, _p(lr_dev), _stream()), "adam_step")


def ema_step(ema, p, ema_bf16, n, one_minus_decay):
    """ema <- ema - (ema - p) * one_minus_decay over n fp32 elements (tf.train.ExponentialMovingAverage); ema_bf16 (optional)
    takes bf16(new ema).  Three separately rounded fp32 operations per element."""
    _dev(ema, p, ema_bf16)
    assert ema.dtype == torch.float32 and p.dtype == torch.float32 and ema.numel() >= n and p.numel() >= n
    assert ema_bf16 is None or (ema_bf16.dtype == torch.bfloat16 and ema_bf16.numel() >= n)
    _check(lib().dmi_ema_step(_p(ema), _p(p), _p(ema_bf16), int(n), float(one_minus_decay), _stream()), "ema_step")


AF_FIELDS = _H.constants["DMI_AF_FIELDS"]   # int64 per variable in an Adafactor descriptor table


def adafactor_plan(table):
    """table: int64 CPU tensor [nvars, AF_FIELDS] with fields 0..8 filled (include/dalle_hip.h K9b); fills fields 9..16 in place
    and returns (tiles, segments, workspace bytes)"""
    assert table.dtype == torch.int64 and not table.is_cuda and table.is_contiguous() and table.shape[1] == AF_FIELDS
    totals = torch.zeros(3, dtype=torch.int64)
    _check(lib().dmi_adafactor_plan(_p(table), table.shape[0], _p(totals)), "adafactor_plan")
    return tuple(int(x) for x in totals)


def adafactor_step(table_dev, nvars, totals, p, g, m, slots, p_bf16, gnorm_sq, clip, lr, decay, beta1, eps1, eps2, ws,
                   lr_dev=None):
    """one Adafactor step over every variable of the planned table (six launches); totals: the tuple adafactor_plan returned"""
    _dev(table_dev, p, g, m, slots, gnorm_sq, ws)
    tot = (ctypes.c_int64 * 3)(*totals)
    _check(lib().dmi_adafactor_step(_p(table_dev), nvars, ctypes.addressof(tot), _p(p), _p(g), _p(m), _p(slots), _p(p_bf16),
                                    _p(gnorm_sq), clip, lr, _p(lr_dev), decay, beta1, eps1, eps2, _p(ws), ws.numel() * ws.element_size(),
                                    _stream()), "adafactor_step")


def cast_f32_bf16(inp, out, n):
    _dev(inp, out)
    _check(lib().dmi_cast_f32_bf16(_p(inp), _p(out), n, _stream()), "cast_f32_bf16")


# ------------------------------------------------------------------ VAE wrappers

def transpose_padded(inp, out, R_valid, R_pitch, C):
    _dev(inp, out)
    _check(lib().dmi_transpose_bf16_padded(_p(inp), _p(out), R_valid, R_pitch, C, _stream()), "transpose_padded")


def _iarr(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def conv_gemm_nt(x, B, H, W, C, Ho, Wo, stride, taps, Wt, ldw, out, ldc, N, flags=0, bias=None, residual=None, relu_src=None):
    """implicit-im2col convolution GEMM (include/dalle_hip.h: dmi_conv_gemm_nt); taps = [(dy, dx), ...]; C % 64 == 0."""
    _dev(x, Wt, out)
    dy, dx = _iarr([t[0] for t in taps]), _iarr([t[1] for t in taps])
    _check(lib().dmi_conv_gemm_nt(_p(x), B, H, W, C, Ho, Wo, stride, len(taps), ctypes.cast(dy, c_void_p),
                                  ctypes.cast(dx, c_void_p), _p(Wt), ldw, _p(out), ldc, N, flags,
                                  _p(bias), _p(residual), _p(relu_src), _stream()), "conv_gemm_nt")


def conv_wgrad_tn_workspace_bytes(M, K, N):
    return int(lib().dmi_conv_wgrad_tn_workspace_bytes(M, K, N))


def conv_wgrad_tn(x, B, H, W, C, Ho, Wo, stride, taps, dY, ldy, N, dW, ws, dbias=None, deferred: "DeferredReduces" = None):
    """implicit-im2col weight gradient (include/dalle_hip.h: dmi_conv_wgrad_tn); Ho, Wo powers of two, C % 64 == 0.
    deferred: as gemm_tn (ws must then be exclusive to this call until deferred.run())."""
    _dev(x, dY, dW, ws)
    dy, dx = _iarr([t[0] for t in taps]), _iarr([t[1] for t in taps])
    if deferred is None:
        _check(lib().dmi_conv_wgrad_tn(_p(x), B, H, W, C, Ho, Wo, stride, len(taps), ctypes.cast(dy, c_void_p),
                                       ctypes.cast(dx, c_void_p), _p(dY), ldy, N, _p(dW), _p(dbias), _p(ws), None, None, _stream()),
               "conv_wgrad_tn")
        return
    assert deferred.n + 2 <= deferred.capacity
    cnt = c_int(0)
    slot = ctypes.byref(deferred.items, deferred.n * ctypes.sizeof(ReduceItem))
    _check(lib().dmi_conv_wgrad_tn(_p(x), B, H, W, C, Ho, Wo, stride, len(taps), ctypes.cast(dy, c_void_p),
                                   ctypes.cast(dx, c_void_p), _p(dY), ldy, N, _p(dW), _p(dbias), _p(ws), slot, ctypes.byref(cnt),
                                   _stream()), "conv_wgrad_tn")
    deferred.n += cnt.value


def im2col(x, out, B, H, W, C, Ho, Wo, stride, taps, ldo):
    """taps: list of (dy, dx) host tuples."""
    _dev(x, out)
    dy, dx = _iarr([t[0] for t in taps]), _iarr([t[1] for t in taps])
    _check(lib().dmi_im2col(_p(x), _p(out), B, H, W, C, Ho, Wo, stride, len(taps), ctypes.cast(dy, c_void_p),
                            ctypes.cast(dx, c_void_p), ldo, _stream()), "im2col")


def weight_gather(inp, out, A, Bn, idx, ldo):
    _dev(inp, out)
    ia = _iarr(idx)
    _check(lib().dmi_weight_gather(_p(inp), _p(out), A, Bn, len(idx), ctypes.cast(ia, c_void_p), ldo, _stream()), "weight_gather")


def pixel_interleave(in4, out, B, Ht, Wt, C):
    _dev(in4, out)
    _check(lib().dmi_pixel_interleave(_p(in4), _p(out), B, Ht, Wt, C, _stream()), "pixel_interleave")


def pad_channels(inp, out, N, Cin, Cp):
    _dev(inp, out)
    _check(lib().dmi_pad_channels(_p(inp), _p(out), N, Cin, Cp, _stream()), "pad_channels")


def unpad_channels(inp, out, N, Cin, Cp):
    _dev(inp, out)
    _check(lib().dmi_unpad_channels(_p(inp), _p(out), N, Cin, Cp, _stream()), "unpad_channels")


def weight_gather_batch(in_base, out_base, table, n, total_blocks):
    _dev(in_base, out_base, table)
    _check(lib().dmi_weight_gather_batch(_p(in_base), _p(out_base), _p(table), n, total_blocks, _stream()), "weight_gather_batch")


def gumbel_softmax_fwd(logits, u, y, y_soft, index, M, T, temperature, hard, temperature_dev=None):
    _dev(logits, u, y, y_soft, index)
    _check(lib().dmi_gumbel_softmax_fwd(_p(logits), _p(u), _p(y), _p(y_soft), _p(index), M, T, float(temperature), int(bool(hard)),
                                        _p(temperature_dev), _stream()), "gumbel_softmax_fwd")


def gumbel_softmax_bwd(dy, y_soft, dlogits, M, T, temperature, temperature_dev=None):
    _dev(dy, y_soft, dlogits)
    _check(lib().dmi_gumbel_softmax_bwd(_p(dy), _p(y_soft), _p(dlogits), M, T, float(temperature), _p(temperature_dev), _stream()),
           "gumbel_softmax_bwd")


def codebook_kl_workspace_bytes(M, T):
    return lib().dmi_codebook_kl_workspace_bytes(M, T)


def codebook_kl_fwd(logits, rowstat, kl, M, T, ws):
    _dev(logits, rowstat, kl, ws)
    _check(lib().dmi_codebook_kl_fwd(_p(logits), _p(rowstat), _p(kl), M, T, _p(ws), _stream()), "codebook_kl_fwd")


def gumbel_softmax_bwd_kl(dy, y_soft, logits, rowstat, dlogits, M, T, temperature, kl_weight, temperature_dev=None,
                          kl_weight_dev=None):
    _dev(dy, y_soft, logits, rowstat, dlogits, temperature_dev, kl_weight_dev)
    _check(lib().dmi_gumbel_softmax_bwd_kl(_p(dy), _p(y_soft), _p(logits), _p(rowstat), _p(dlogits), M, T, float(temperature),
                                           _p(temperature_dev), float(kl_weight), _p(kl_weight_dev), _stream()),
           "gumbel_softmax_bwd_kl")


def elbo_loss(recon, kl, loss, kl_weight, kl_weight_dev=None):
    _dev(recon, kl, loss, kl_weight_dev)
    _check(lib().dmi_elbo_loss(_p(recon), _p(kl), float(kl_weight), _p(kl_weight_dev), _p(loss), _stream()), "elbo_loss")


def codebook_usage(logits, rowstat, index, qsum, counts, M, T, ws):
    _dev(logits, rowstat, index, qsum, counts, ws)
    _check(lib().dmi_codebook_usage(_p(logits), _p(rowstat), _p(index), _p(qsum), _p(counts), M, T, _p(ws), _stream()),
           "codebook_usage")


def vq_half_norms(h, T, D, codebook_t=None, ldc=0, codebook_f32=None):
    """h[k] = 1/2 sum_j c[j,k]^2 from the bf16 transpose [T, ldc] or from the fp32 masters [D, T] (exactly one)"""
    _dev(h, codebook_t, codebook_f32)
    _check(lib().dmi_vq_half_norms(_p(codebook_t), ldc, _p(codebook_f32), _p(h), T, D, _stream()), "vq_half_norms")


def vq_assign(x, ldx, codebook_t, ldc, h, idx, xq, ldq, score, M, T, D):
    _dev(x, codebook_t, h, idx, xq, score)
    _check(lib().dmi_vq_assign(_p(x), ldx, _p(codebook_t), ldc, _p(h), _p(idx), _p(xq), ldq, _p(score), M, T, D, _stream()), "vq_assign")


def vq_scores_bias(scores, h, M, T):
    _dev(scores, h)
    _check(lib().dmi_vq_scores_bias(_p(scores), _p(h), M, T, _stream()), "vq_scores_bias")


def vq_loss_workspace_bytes():
    return lib().dmi_vq_loss_workspace_bytes()


def vq_loss(x, ldx, xq, ldq, loss, M, D, ws):
    _dev(x, xq, loss, ws)
    _check(lib().dmi_vq_loss(_p(x), ldx, _p(xq), ldq, _p(loss), M, D, _p(ws), _stream()), "vq_loss")


def vq_bwd_x(d, ldd, x, ldx, xq, ldq, dx, lddx, M, D, beta):
    _dev(d, x, xq, dx)
    _check(lib().dmi_vq_bwd_x(_p(d), ldd, _p(x), ldx, _p(xq), ldq, _p(dx), lddx, M, D, float(beta), _stream()), "vq_bwd_x")


def vq_codebook_grad_workspace_bytes(M, T, D):
    return lib().dmi_vq_codebook_grad_workspace_bytes(M, T, D)


def vq_codebook_grad(x, ldx, idx, codebook_t, ldc, dC, M, T, D, ws=None):
    _dev(x, idx, codebook_t, dC, ws)
    _check(lib().dmi_vq_codebook_grad(_p(x), ldx, _p(idx), _p(codebook_t), ldc, _p(dC), M, T, D, _p(ws), _stream()), "vq_codebook_grad")


def vq_gather(codebook_t, ldc, idx, out, ldo, M, T, D):
    _dev(codebook_t, idx, out)
    _check(lib().dmi_vq_gather(_p(codebook_t), ldc, _p(idx), _p(out), ldo, M, T, D, _stream()), "vq_gather")


def vq_cluster_sums_workspace_bytes(M, T, D):
    return int(lib().dmi_vq_cluster_sums_workspace_bytes(M, T, D))


def vq_cluster_sums(x, ldx, idx, sums, counts, M, T, D, ws=None):
    """counts[k] = #{m : idx[m] = k}; sums[k, :] = the fp32 sum of the rows x[m, :] with idx[m] = k, in a fixed order ([T, D])"""
    _dev(x, idx, sums, counts, ws)
    _check(lib().dmi_vq_cluster_sums(_p(x), ldx, _p(idx), _p(sums), _p(counts), M, T, D, _p(ws), _stream()), "vq_cluster_sums")


def vq_ema_step(codebook_f32, codebook_bf16, N, S, idle, restarts, sums, counts, x, ldx, gamma, restart_after, seed, step, M, T, D,
                step_dev=None):
    """EMA update of N, S and the codebook from this step's cluster sums, then the dead-code restarts (include/dalle_hip.h)"""
    _dev(codebook_f32, codebook_bf16, N, S, idle, restarts, sums, counts, x, step_dev)
    _check(lib().dmi_vq_ema_step(_p(codebook_f32), _p(codebook_bf16), _p(N), _p(S), _p(idle), _p(restarts), _p(sums), _p(counts), _p(x), ldx,
                                 float(gamma), int(restart_after), int(seed) & 0xFFFFFFFFFFFFFFFF, int(step), _p(step_dev), M, T, D, _stream()),
           "vq_ema_step")


def mse_workspace_bytes():
    return lib().dmi_mse_workspace_bytes()


def mse_loss(img, outp, dout, loss, N, Cin, Cp, grad_scale, ws):
    _dev(img, outp, dout, loss, ws)
    _check(lib().dmi_mse_loss(_p(img), _p(outp), _p(dout), _p(loss), N, Cin, Cp, float(grad_scale), _p(ws), _stream()), "mse_loss")


def add_f32(dst, src, n):
    _dev(dst, src)
    _check(lib().dmi_add_f32(_p(dst), _p(src), n, _stream()), "add_f32")


def conv2d_f32(x, B, H, W, C, Ho, Wo, stride, taps, Wk, bias, residual, out, N, relu=False):
    """fp32 convolution on the exact-fp32 matrix cores (tokenising encoder); taps = [(dy, dx), ...]."""
    _dev(x, Wk, bias, residual, out)
    dy, dx = _iarr([t[0] for t in taps]), _iarr([t[1] for t in taps])
    _check(lib().dmi_conv2d_f32(_p(x), B, H, W, C, Ho, Wo, stride, len(taps), ctypes.cast(dy, c_void_p), ctypes.cast(dx, c_void_p),
                                _p(Wk), _p(bias), _p(residual), _p(out), N, int(bool(relu)), _stream()), "conv2d_f32")


def space_to_depth_f32(img, stacked, B, Hs, Ws, C, s, Cp):
    _dev(img, stacked)
    _check(lib().dmi_space_to_depth_f32(_p(img), _p(stacked), B, Hs, Ws, C, s, Cp, _stream()), "space_to_depth_f32")


def depth_to_space_f32(stacked, img, B, Hs, Ws, C, s, Cp):
    _dev(stacked, img)
    _check(lib().dmi_depth_to_space_f32(_p(stacked), _p(img), B, Hs, Ws, C, s, Cp, _stream()), "depth_to_space_f32")


# ------------------------------------------------------------------ data-parallel exchange (RCCL behind the C ABI)

def comm_load():
    """bind the librccl this process already maps (PyTorch-ROCm ships its own copy) or the system one."""
    cand = os.path.join(os.path.dirname(torch.__file__), "lib", "librccl.so")
    path = os.environ.get("DALLE_RCCL_LIB") or (cand if os.path.exists(cand) else "")
    _check(lib().dmi_comm_load(path.encode()), "comm_load")


def comm_unique_id() -> bytes:
    comm_load()
    buf = ctypes.create_string_buffer(lib().dmi_comm_unique_id_bytes())
    _check(lib().dmi_comm_unique_id(ctypes.cast(buf, c_void_p)), "comm_unique_id")
    return buf.raw


def comm_init(nranks: int, rank: int, unique_id: bytes) -> int:
    """blocking collective; returns the opaque communicator handle (int)."""
    comm_load()
    out = c_void_p()
    buf = ctypes.create_string_buffer(unique_id, len(unique_id))
    _check(lib().dmi_comm_init(ctypes.byref(out), nranks, rank, ctypes.cast(buf, c_void_p)), "comm_init")
    return out.value


def comm_destroy(comm):
    if comm:
        _check(lib().dmi_comm_destroy(c_void_p(comm)), "comm_destroy")


def allreduce_bucket(comm, g, n, stream=None):
    _dev(g)
    _check(lib().dmi_allreduce_bucket(c_void_p(comm), _p(g), n, _stream() if stream is None else stream), "allreduce_bucket")


def comm_broadcast_f32(comm, buf, n, root=0, stream=None):
    _dev(buf)
    _check(lib().dmi_comm_broadcast_f32(c_void_p(comm), _p(buf), n, root, _stream() if stream is None else stream), "comm_broadcast")
