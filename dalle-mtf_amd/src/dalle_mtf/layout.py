"""The flat parameter layout of the DALL-E engine and what is derived from it on the host: the reference's variable table
 and Adafactor's descriptor table.  Pure CPU code: nothing here touches a device."""
from __future__ import annotations

import math
from collections import OrderedDict
from typing import Dict, List, Tuple

import numpy as np
import torch

from .ff_glu import ffn1_width
from .qk_norm import GAIN_NAMES

ALIGN = 128  # elements


def _round_up(x, m):
    return (x + m - 1) // m * m


def adafactor_factored_dims(shape, min_dim_size_to_factor=128):
    """mtf AdafactorOptimizer._factored_dims (mesh-tensorflow 0.1.18 optimize.py, restated from memory: no mesh-tensorflow was
    available to check it against): None below rank 2; otherwise the axes sorted by size, descending and stable (ties keep axis
    order), d0 = the largest, d1 = the second -- None when d1 is smaller than min_dim_size_to_factor.  Returns (d0, d1) axes."""
    if len(shape) < 2:
        return None
    order = sorted(range(len(shape)), key=lambda i: -shape[i])
    if shape[order[1]] < min_dim_size_to_factor:
        return None
    return order[0], order[1]


def adafactor_table(lay):
    """the Adafactor descriptor table of a ParamLayout (fields 0..8 of include/dalle_hip.h K9b; dmi_adafactor_plan fills the
    rest), one row per reference variable, the per-variable slot records and the slot buffer's length.  Slots: the row vector [R]
    and the column vector [C] of a factored variable, the dense v [R, C] otherwise, in 16-byte aligned pieces."""
    rows, recs, so = [], [], 0
    for name, shp, off, ld in lay.reference_variables():
        R, C = (1, shp[0]) if len(shp) == 1 else shp
        fd = adafactor_factored_dims(shp)
        rec = dict(name=name, shape=shp, factored=fd is not None)
        if fd is not None:
            rec["row"], rec["col"] = so, so + _round_up(R, 4)
            so += _round_up(R, 4) + _round_up(C, 4)
            rec["vr_row"] = fd[0] == 1       # vr is indexed along d1: the rows when d0 is the column axis
            rows.append([off, R, C, ld, 1, int(rec["vr_row"]), rec["row"], rec["col"], 0] + [0] * 8)
        else:
            rec["v"] = so
            so += _round_up(R * C, 4)
            rows.append([off, R, C, ld, 0, 0, 0, 0, rec["v"]] + [0] * 8)
        recs.append(rec)
    return torch.tensor(rows, dtype=torch.int64), recs, so


class ParamLayout:
    """Flat layout of the trainable variables.  Internal tensors fuse q|k|v into one [d, 3d] matrix and
    pad the vocabulary axis of the output projection to a multiple of 128; `export`/`load` translate
    to/from the reference's variable names and shapes."""

    def __init__(self, n_embd, n_layers, n_heads, total_tokens, total_seq, ff_glu=False, qk_norm=False):
        d, L, V, S = n_embd, n_layers, total_tokens, total_seq
        self.d, self.L, self.V, self.S = d, L, V, S
        # mlp_linear_1's output width: 4d, or with the gated FFN (config key "ff_glu") [value | gate] = 8d; everything derived from
        # the entries -- the transposed-copy table, the reference's variable table, Adafactor's, reference_init -- follows it
        self.ff_glu = bool(ff_glu)
        f1 = self.ffn1 = ffn1_width(d, self.ff_glu)
        # QK normalisation (config key "qk_norm"): two [head_dim] gains per layer, shared by its heads, between attn/qkv and norm_1/g
        # -- inside the layer's bucket, so bucket_ends and ready_points keep their meaning; off: the entries are exactly the plain ones
        self.qk_norm = bool(qk_norm)
        qkn = [(g, (d // n_heads,)) for g in GAIN_NAMES] if self.qk_norm else []
        self.Vp = _round_up(V, 128)
        ent: List[Tuple[str, tuple]] = []
        ent += [("to_logits/linear_out/kernel", (d, self.Vp)), ("to_logits/linear_out/bias", (self.Vp,)),
                ("to_logits/layer_norm/g", (d,)), ("to_logits/layer_norm/b", (d,))]
        for i in reversed(range(L)):
            p = f"layer_{i}/"
            ent += [(p + "mlp/mlp_linear_2/kernel", (4 * d, d)), (p + "mlp/mlp_linear_2/bias", (d,)),
                    (p + "mlp/mlp_linear_1/kernel", (d, f1)), (p + "mlp/mlp_linear_1/bias", (f1,)),
                    (p + "norm_2/g", (d,)), (p + "norm_2/b", (d,)),
                    (p + "attn/o", (d, d)), (p + "attn/compute_output_bias/o_b", (d,)),
                    (p + "attn/qkv", (d, 3 * d))]
            ent += [(p + g, shp) for g, shp in qkn]
            ent += [(p + "norm_1/g", (d,)), (p + "norm_1/b", (d,))]
        ent += [("positional_embedding/wpe", (S, d)), ("embedding/wte", (V, d))]
        self.entries = ent
        self.offset: Dict[str, int] = {}
        self.shape: Dict[str, tuple] = {}
        off = 0
        for name, shp in ent:
            self.offset[name] = off
            self.shape[name] = shp
            off += _round_up(int(np.prod(shp)), ALIGN)
        self.total = off
        # transposed ([out, in]) bf16 copies consumed by the forward GEMMs
        self.t_offset: Dict[str, int] = {}
        toff = 0
        for name, shp in ent:
            if len(shp) == 2 and ("kernel" in name or "attn/" in name):
                self.t_offset[name] = toff
                toff += _round_up(int(np.prod(shp)), ALIGN)
        self.t_total = toff
        # bucket boundaries (prefix ends) in element offsets: after head, after each layer, end
        self.bucket_ends: List[int] = []
        self.bucket_ends.append(self.offset[f"layer_{L-1}/mlp/mlp_linear_2/kernel"] if L > 0 else self.offset["positional_embedding/wpe"])
        for i in reversed(range(L)):
            nxt = f"layer_{i-1}/mlp/mlp_linear_2/kernel" if i > 0 else "positional_embedding/wpe"
            self.bucket_ends.append(self.offset[nxt])
        self.bucket_ends.append(self.total)
        # offsets at which backward has finished a prefix of the flat gradient buffer, in completion order: the head's
        # kernel + bias (right after its weight-gradient GEMM, before the input gradient), each layer (the head LayerNorm's
        # gain / bias ride with layer L-1), finally the embeddings.  The exchange pieces follow these cuts (src/dp.py).
        self.ready_points: List[int] = [self.offset["to_logits/layer_norm/g"]] + self.bucket_ends[1:]

    def numel(self, name):
        return int(np.prod(self.shape[name]))

    def reference_variables(self):
        """the reference's variables in flat-buffer order as (name, shape, offset, leading dimension):
        q / k / v are column blocks of the fused [d, 3d] matrix; the head's kernel and bias keep V of their Vp columns"""
        out = []
        for name, shp in self.entries:
            o = self.offset[name]
            if name.endswith("attn/qkv"):
                base = name[:-3]
                out += [(base + t, (self.d, self.d), o + i * self.d, 3 * self.d) for i, t in enumerate("qkv")]
            elif name == "to_logits/linear_out/kernel":
                out.append((name, (self.d, self.V), o, self.Vp))
            elif name == "to_logits/linear_out/bias":
                out.append((name, (self.V,), o, self.V))
            else:
                out.append((name, shp, o, shp[-1]))
        return out


def reference_init(lay, n_heads, seed=1234):
    """the reference's initial values of every variable of a ParamLayout: LayerNorm gains 1, biases 0, the
    matrices normal with the standard deviations below, drawn with torch's generator in the order embeddings, layer 0 .. L-1
    (q, k, v, o, mlp_linear_1, mlp_linear_2), output projection -- the draws' order fixes the values"""
    d, k = lay.d, lay.d // n_heads
    std = {"embedding/wte": 0.02, "positional_embedding/wpe": 0.01, "to_logits/linear_out/kernel": 0.02,
           "attn/q": (d * k) ** -0.5, "attn/k": d ** -0.5, "attn/v": d ** -0.5, "attn/o": (n_heads * k) ** -0.5,
           "mlp/mlp_linear_1/kernel": 0.02, "mlp/mlp_linear_2/kernel": 0.02 / math.sqrt(lay.L) if lay.L else 0.0}
    drawn = (["embedding/wte", "positional_embedding/wpe"] + [f"layer_{i}/{t}" for i in range(lay.L) for t in list(std)[3:]]
             + ["to_logits/linear_out/kernel"])
    P = OrderedDict((name, (np.ones if name.endswith("/g") else np.zeros)(shp, np.float32)) for name, shp, _, _ in lay.reference_variables())
    g = torch.Generator().manual_seed(seed)
    for name in drawn:
        P[name] = (torch.randn(*P[name].shape, generator=g) * std[name.split("/", 1)[1] if name.startswith("layer_") else name]).numpy()
    return P
