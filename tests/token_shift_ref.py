"""References for token shift (dalle_mtf.token_shift, dmi_token_shift):
  shift64         the float64 shift (or its transpose) of [rows, d] rows, a gather built from shift_sources -- what the kernels
                  are held to, bit for bit;
  shift           the same shift of a torch [B, S, d] tensor, written with slices and pads so that autograd differentiates it --
                  what the fp32 step oracle (tests/dalle_step_ref.py, token_shift=) puts behind both LayerNorms of every block."""
import numpy as np
import torch
import torch.nn.functional as F

from src.dalle_mtf.token_shift import shift_sources


def shift64(x, T, G, inverse=False):
    """x [rows, d] (any float dtype; rows a multiple of S = T + G * G) -> its float64 shift, or the transpose"""
    x = np.asarray(x, np.float64)
    rows, d = x.shape
    S = T + G * G
    assert rows % S == 0
    src = shift_sources(T, G, d, inverse=inverse)                              # [S, d]
    x3 = x.reshape(rows // S, S, d)
    got = np.take_along_axis(x3, np.broadcast_to(np.maximum(src, 0), x3.shape), axis=1)
    return np.where(src[None] >= 0, got, 0.0).reshape(rows, d)


def shift(x, T, G):
    """x [B, S, d] torch -> shift(x), differentiable: the caption rows move down by one; the image grid moves down by one row for
    the first quarter and right by one column for the second"""
    B, S, d = x.shape
    q = d // 4
    text, img = x[:, :T], x[:, T:].reshape(B, G, G, d)
    text_s = F.pad(text[:, :-1, :2 * q], (0, 0, 1, 0))                         # [B, T, d/2]
    up = F.pad(img[:, :-1, :, :q], (0, 0, 0, 0, 1, 0))                         # from above
    left = F.pad(img[:, :, :-1, q:2 * q], (0, 0, 1, 0))                        # from the left
    img_s = torch.cat([up, left], dim=-1).reshape(B, G * G, 2 * q)
    return torch.cat([torch.cat([text_s, img_s], dim=1), x[:, :, 2 * q:]], dim=-1)
