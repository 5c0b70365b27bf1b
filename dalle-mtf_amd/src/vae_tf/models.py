"""DiscreteVAE -- same constructor / forward surface as the reference (src/vae_tf/models.py:46-184), re-hosted on
libdalle_hip: every convolution is a tap list feeding the MFMA GEMMs -- gathered implicitly inside the GEMM
(dmi_conv_gemm_nt / dmi_conv_wgrad_tn) for 64-channel-aligned layers, through a materialised im2col (dmi_im2col +
dmi_gemm_nt / dmi_gemm_tn) otherwise, as lowering.py states per layer and _tap_product / _tap_wgrad launch; Gumbel-softmax and
MSE are dedicated kernels (csrc/vae.hip).  bf16 activations/weights, fp32 accumulation, fp32
master weights and Adam state; the codebook logits are produced in fp32 (reference: fp32 matmul, models.py:113-118).

Layer structure (reference lines): encoder 81-120: per block a 4x4 s2 SAME conv (no activation) then (stack-1) x
`x + conv3x3(relu(conv3x3(x)))`; fp32 `x @ codebook`.  decoder 123-163: `y @ codebook^T` (tied), per reversed block a
4x4 s2 conv-transpose (no activation) then the residual stacks, final 1x1 conv.  forward 165-184.

Internal tensor conventions: activations NHWC as [B*H*W, C] bf16; the 3-channel image is padded to 8 channels and the
3-channel reconstruction to 64 so that every GEMM keeps K % 64 == 0 / N % 8 == 0; the corresponding kernel rows /
columns are zero and stay zero (their gradients are exactly 0).  `export_reference` / `load_reference_params`
translate to the TF variable names and shapes of SURVEY.md Appendix B.
"""
from __future__ import annotations

import math
import os
from collections import OrderedDict
from typing import Dict

import numpy as np
import torch

import dalle_hip as dh
from ..dp import GradReducer
from . import lowering
from .lowering import OUT_CP, TAPS3, _Conv, _ru   # noqa: F401  (TAPS3: the tests read it from here)
from .kl import _perplexity, kl_weight_at, resolve_kl_options, usage_stats
from .vq import check_checkpoint, resolve_vq_options
from .vq_ema import STATE_KEYS as VQ_EMA_STATE_KEYS, check_checkpoint as check_ema_checkpoint, resolve_vq_ema_options

VQ_MAX_WIDTH = 512           # widest code of dmi_vq_assign / dmi_vq_codebook_grad
GUMBEL_MAX_TOKENS = 4096    # largest codebook of dmi_gumbel_softmax_fwd (eight 8-column chunks per lane)
WS_POOL = 7    # weight gradients in flight before their slab reduces are flushed (2 reduce items each, 16 per batched launch)


class DiscreteVAE:
    def __init__(self, num_tokens, dimensions, convblocks, dim=512, hidden_dim=64, input_channels=3, recompute_grad=False,
                 use_bf16=False, stack_factor=1, batch_size=32, mode="train", device="cuda", process_group=None, world_size=1,
                 comm=None, kl_loss_weight=0.0, kl_anneal_steps=None, quantizer=None, vq_commitment=None, vq_ema_decay=None, vq_restart_after=None,
                 vq_restart_seed=None):
        kl = resolve_kl_options(dict(kl_loss_weight=kl_loss_weight, kl_anneal_steps=kl_anneal_steps))   # ValueError before any device work
        vq = resolve_vq_options(dict(quantizer=quantizer, vq_commitment=vq_commitment, kl_loss_weight=kl_loss_weight,
                                     kl_anneal_steps=kl_anneal_steps))
        ema = resolve_vq_ema_options(dict(quantizer=quantizer, vq_ema_decay=vq_ema_decay, vq_restart_after=vq_restart_after,
                                          vq_restart_seed=vq_restart_seed), world=world_size)
        if num_tokens > GUMBEL_MAX_TOKENS:
            raise ValueError(f"num_tokens = {num_tokens}: the Gumbel-softmax kernel (dmi_gumbel_softmax_fwd, one wave per row) "
                             f"handles codebooks of at most {GUMBEL_MAX_TOKENS} tokens")
        n_hid = tuple(convblocks[-1])[1]
        if vq.quantizer == "vq" and (n_hid % 64 != 0 or not 64 <= n_hid <= VQ_MAX_WIDTH):
            raise ValueError(f"quantizer = 'vq': the code width n_hid = {n_hid} (the last convblock's channels) must be a multiple of 64 "
                             f"between 64 and {VQ_MAX_WIDTH} (dmi_vq_assign keeps 64 rows of that width in LDS)")
        if not torch.cuda.is_available():
            raise dh.DalleHipError("DiscreteVAE needs a HIP device (MI355X); there is no CPU fallback")
        dh.lib()
        self.num_tokens = num_tokens
        self.dim, self.hdim = dim, hidden_dim
        self.num_ch = input_channels
        self.H = self.W = dimensions
        self.convblocks = [tuple(b) for b in convblocks]
        self.recompute_grad = recompute_grad     # memory-only option: residual branches are re-run in backward()
        self.bf16 = use_bf16                     # kernels always compute in bf16 with fp32 accumulation
        assert math.log2(stack_factor).is_integer()
        # tf.space_to_depth in front of the encoder / tf.depth_to_space behind the decoder (reference :85-86,158-161): the
        # network runs on [B, H/s, W/s, C*s*s]; two index kernels do the re-layout, everything else is unchanged
        self.stack_factor = stack_factor
        assert dimensions % stack_factor == 0
        self.Hs = dimensions // stack_factor                 # spatial size the convolutions see
        self.c_st = input_channels * stack_factor ** 2       # channels after space_to_depth
        self.img_cp = _ru(self.c_st, 8)                      # ... padded for the 16-byte vector paths
        assert self.c_st <= OUT_CP, "stack_factor too large for the padded reconstruction width"
        self.fp32_tokens = False   # return_logits path on the exact-fp32 kernels (set by dalle_model_fn's load_vae_model)
        for _, ch in self.convblocks:
            assert ch % 16 == 0, "channel counts must be multiples of 16"
        assert num_tokens % 64 == 0, "num_tokens must be a multiple of 64"
        assert self.convblocks[-1][1] % 64 == 0, "the last block's channel count (codebook width) must be a multiple of 64"
        self.B, self.mode = batch_size, mode
        self.dev = torch.device(device)
        self.pg, self.world = process_group, world_size
        self.n_hid = self.convblocks[-1][1]
        self.grid = self.Hs // (2 ** len(self.convblocks))
        self.global_step = 0
        # loss = recon + beta_t KL(q || uniform), beta_t = beta min(1, step / kl_anneal_steps) (vae_tf/kl.py; 0 = the reference's loss)
        self.kl_weight, self.kl_anneal_steps = kl.kl_loss_weight, kl.kl_anneal_steps
        self.kl_weight_t = self.kl_weight if kl.kl_anneal_steps is None else 0.0
        self.rowstat = self.loss_recon = self.loss_kl = self.ws_kl = self._usage = None
        # "vq": nearest-code bottleneck, loss = recon + (1 + beta) Lq (vae_tf/vq.py); "gumbel" = the reference's, unchanged
        self.quantizer, self.vq_on, self.vq_beta = vq.quantizer, vq.quantizer == "vq", vq.vq_commitment
        # "vq_ema_decay": the codebook follows its clusters' moving averages instead of a gradient, loss = recon + beta Lq (vae_tf/vq_ema.py)
        self.vq_ema_decay, self.vq_restart_after, self.vq_restart_seed = ema
        self.vq_ema = None           # N, S, idle, restarts (_alloc) when vq_ema_decay is set
        self._kl_fresh = False       # rowstat / loss_kl describe the logits buffer as it stands
        self._graphs, self._graph_warm, self._dyn_on, self._img_static = {}, False, False, None
        self.event_hook = None       # (layer name, list): HIP event pairs around that layer's implicit forward launch (bench.py)
        self._f32 = None             # scratch of encode_logits_fp32, at its first call
        self._build_graph()
        self._alloc()
        self._dyn = torch.zeros(3, dtype=torch.float32, device=self.dev)   # [lr_t, temperature, beta_t] read by graph-replayed kernels
        # gradient exchange (mean over replicas = SUM here x grad_scale 1/world in the Adam kernel), overlapped with backward
        self.reducer = GradReducer(self.g, world_size, comm=comm, pg=process_group)

    # ------------------------------------------------------------------ structure
    def _build_graph(self):
        """the layer list with every layer's tap products and the flat parameter layout (lowering.py)"""
        self.convs, self.n_enc, self.offset, self.shape, self.total = lowering.build_graph(
            self.Hs, self.img_cp, self.c_st, self.convblocks, self.n_hid, self.num_tokens)

    def _alloc(self):
        B, dev = self.B, self.dev
        b16 = dict(dtype=torch.bfloat16, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        n = self.total
        self.p, self.g = torch.zeros(n, **f32), torch.zeros(n, **f32)
        self.m, self.v = torch.zeros(n, **f32), torch.zeros(n, **f32)
        self.pb = torch.zeros(n, **b16)
        # second contribution to the tied codebook gradient (the VQ codebook gradient has one source)
        self.gc2 = None if self.vq_on else torch.zeros(self.n_hid * self.num_tokens, **f32)
        # derived weight copies: views of ONE flat buffer, so that the per-step refresh is two batched launches
        # (dmi_transpose_bf16_batch + dmi_weight_gather_batch) instead of one launch per copy
        self.wf, self.wd, self.wp = {}, {}, {}
        plan, self._wc_off, size = lowering.weight_copies(self.convs, self.n_hid, self.num_tokens)
        self.wcopies = torch.zeros(size, **b16)
        for kind, name, q, rows, cols in plan:
            o = self._wc_off[(kind, name, q)]
            v = self.wcopies[o:o + rows * cols].view(rows, cols)
            if kind == "wp":
                self.wp.setdefault(name, [None] * 4)[q] = v
            elif kind == "cb":
                self.codebook_t = v
            else:
                getattr(self, kind)[name] = v
        self._refresh_tables = None
        self.col = torch.empty(lowering.max_col(self.convs, B), **b16)    # sized over the implicit products too
        # im2col matrices of the forward convolutions kept for their weight gradients (288 GB HBM: ~8 GB for vae_coco at 16
        # images) -- the backward pass then gathers only dy; allocated on first use in train mode
        self.col_keep = {}
        self._col_valid = set()
        self.keep_cols = (self.mode == "train")
        # activations
        self.x_img = torch.empty(B * self.Hs * self.Hs, self.img_cp, **b16)
        self.img_st = torch.empty(B * self.Hs * self.Hs, self.c_st, **f32) if self.stack_factor > 1 else None
        self.act_in = [None] * len(self.convs)     # input of each conv (kept for the weight gradients)
        self.act_out = []
        # recompute_grad (reference vae_tf/models.py:8-43,102,150): the residual branch is re-run in the backward pass instead of
        # keeping its inner activation -- here: every conv_in output shares ONE buffer, refilled by backward() before use
        shared = None
        if self.recompute_grad:
            shared = torch.empty(max([B * c.Ho * c.Wo * c.cout for c in self.convs if c.name.endswith("conv_in")] + [8]), **b16)
        for c in self.convs:
            if shared is not None and c.name.endswith("conv_in"):
                self.act_out.append(shared[:B * c.Ho * c.Wo * c.cout].view(B * c.Ho * c.Wo, c.cout))
            else:
                self.act_out.append(torch.empty(B * c.Ho * c.Wo, c.cout, **b16))
        Mg = B * self.grid * self.grid
        self.Mg = Mg
        if self.vq_on:      # nothing of size [M, T] in the training step; logits come into being with the first return_logits call
            self.logits = self.u = self.y = self.y_soft = None
            self.h = torch.zeros(self.num_tokens, **f32)              # half-norms of the bf16 codebook (refresh_compute_copies)
            self.h32 = None                                           # ... of the fp32 masters (encode_logits_fp32)
            self.loss_recon, self.loss_vq = torch.zeros(1, **f32), torch.zeros(1, **f32)
            self.ws_vq = torch.empty(int(max(dh.vq_loss_workspace_bytes(), dh.vq_codebook_grad_workspace_bytes(Mg, self.num_tokens, self.n_hid)))
                                     + 1024, dtype=torch.uint8, device=dev)
        else:
            self.logits = torch.empty(Mg, self.num_tokens, **f32)
            self.u = torch.empty(Mg, self.num_tokens, **f32)
            self.y = torch.empty(Mg, self.num_tokens, **b16)
            self.y_soft = torch.empty(Mg, self.num_tokens, **b16)
        if self.vq_ema_decay is not None:       # cluster state, this step's cluster sums, and the step the restart hash reads in a replay
            T, nh = self.num_tokens, self.n_hid
            self.vq_ema = dict(N=torch.ones(T, **f32), S=torch.zeros(T, nh, **f32), idle=torch.zeros(T, dtype=torch.int32, device=dev),
                               restarts=torch.zeros(1, dtype=torch.int32, device=dev))
            self._ema_sums, self._ema_counts = torch.zeros(T, nh, **f32), torch.zeros(T, dtype=torch.int32, device=dev)
            self._ema_ws = torch.empty(int(dh.vq_cluster_sums_workspace_bytes(Mg, T, nh)) + 1024, dtype=torch.uint8, device=dev)
            self._step_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        self.index = torch.empty(Mg, dtype=torch.int32, device=dev)
        self.xdec = torch.empty(Mg, self.n_hid, **b16)
        self.loss = torch.zeros(1, **f32)
        # scratch for parity outputs and gradients
        max_act = max(int(a.numel()) for a in self.act_out + [self.x_img])
        self.par = torch.empty(max_act, **b16)
        self.ga = torch.empty(max_act, **b16)
        self.gb = torch.empty(max_act, **b16)
        self.gc = torch.empty(max_act, **b16)
        self.dy = None if self.vq_on else torch.empty(Mg, self.num_tokens, **b16)
        self.dlogits = None if self.vq_on else torch.empty(Mg, self.num_tokens, **b16)
        bounds = lowering.wgrad_bounds(self.convs, B)      # per layer (M, K, N) of its weight gradient and column sum
        wsz = max([1 << 20] + [max(dh.gemm_tn_workspace_bytes(M, K, N), dh.colsum_workspace_bytes(M, N)) for M, K, N in bounds])
        wsz = max(wsz, dh.gemm_tn_workspace_bytes(Mg, self.n_hid, self.num_tokens), dh.mse_workspace_bytes())
        if self.kl_weight > 0:
            self._kl_buffers()
        self.ws = torch.empty(int(wsz) + 1024, dtype=torch.uint8, device=dev)
        # backward(): the split-m slab reduces of the weight gradients are DEFERRED and run a few layers at a time in one launch
        # (the small configurations spent a fifth of their step in ~60 reduce launches of a few microseconds); every pending
        # weight gradient owns one workspace of this pool until the flush
        self.ws_cs = torch.empty(int(max(dh.colsum_workspace_bytes(M, N) for M, K, N in bounds)) + 1024, dtype=torch.uint8,
                                 device=dev)                                   # column sums reduce at once
        self.ws_pool = [torch.empty_like(self.ws) for _ in range(WS_POOL)]     # (self.ws stays free for the immediate calls)
        self._ws_next = 0
        self.deferred = dh.DeferredReduces()

    def _kl_buffers(self):
        """(lse, e) per row, the two loss terms as device scalars and the workspace of dmi_codebook_kl_fwd / dmi_codebook_usage (sized by
        dmi_codebook_kl_workspace_bytes, as the header asks): with the model when kl_loss_weight > 0, else at the first
        codebook_stats()"""
        if self.rowstat is None:
            f32 = dict(dtype=torch.float32, device=self.dev)
            self.rowstat = torch.empty(self.Mg, 2, **f32)
            self.loss_recon, self.loss_kl = torch.zeros(1, **f32), torch.zeros(1, **f32)
            self.ws_kl = torch.empty(int(dh.codebook_kl_workspace_bytes(self.Mg, self.num_tokens)) + 1024, dtype=torch.uint8, device=self.dev)

    # ------------------------------------------------------------------ parameters
    def view(self, buf, name):
        o = self.offset[name]
        shp = self.shape[name]
        return buf[o:o + int(np.prod(shp))].view(shp)

    def init_params(self, seed=4321):
        """glorot-uniform kernels / codebook, zero biases (tf.layers defaults)."""
        g = torch.Generator().manual_seed(seed)
        P = OrderedDict()
        for name, shp in self.reference_variables().items():
            if len(shp) == 1:
                P[name] = np.zeros(shp, np.float32)
            else:
                if len(shp) == 4:
                    rf = shp[0] * shp[1]
                    fi, fo = shp[2] * rf, shp[3] * rf
                else:
                    fi, fo = shp
                lim = math.sqrt(6.0 / (fi + fo))
                P[name] = ((torch.rand(*shp, generator=g) * 2 - 1) * lim).numpy()
        self.load_reference_params(P)

    def reference_variables(self) -> "OrderedDict[str, tuple]":
        out: "OrderedDict[str, tuple]" = OrderedDict()
        for i, c in enumerate(self.convs):
            if i == self.n_enc:
                out["codebook/codebook"] = (self.n_hid, self.num_tokens)
            k = {16: 4, 9: 3, 1: 1}[c.kk]
            if c.kind == "up":
                out[c.name + "/kernel"] = (k, k, c.cout_ref, c.cin_ref)
            else:
                out[c.name + "/kernel"] = (k, k, c.cin_ref, c.cout_ref)
            out[c.name + "/bias"] = (c.cout_ref,)
        return out

    def load_reference_params(self, P: Dict[str, np.ndarray]):
        with torch.no_grad():
            self.p.zero_()
            for c in self.convs:
                w = torch.from_numpy(np.ascontiguousarray(P[c.name + "/kernel"])).float()
                k = w.shape[0]
                w = w.reshape(k * k, w.shape[2], w.shape[3])
                dst = self.view(self.p, c.name + "/kernel")
                dst[:, :w.shape[1], :w.shape[2]] = w
                bsrc = torch.from_numpy(np.ascontiguousarray(P[c.name + "/bias"])).float()
                self.view(self.p, c.name + "/bias")[:bsrc.shape[0]] = bsrc
            self.view(self.p, "codebook/codebook").copy_(torch.from_numpy(np.ascontiguousarray(P["codebook/codebook"])))
            if self.vq_ema is not None:      # parameters without cluster state: N = 1, S[k] = C[:,k], nothing idle, no restarts yet
                e = self.vq_ema
                e["N"].fill_(1.0); e["S"].copy_(self.view(self.p, "codebook/codebook").t()); e["idle"].zero_(); e["restarts"].zero_()
        self.refresh_compute_copies(cast=True)

    def export_reference(self, buf=None) -> "OrderedDict[str, np.ndarray]":
        buf = self.p if buf is None else buf
        out: "OrderedDict[str, np.ndarray]" = OrderedDict()
        ref = self.reference_variables()
        for c in self.convs:
            shp = ref[c.name + "/kernel"]
            a = self.view(buf, c.name + "/kernel").detach().float().cpu().numpy()
            out[c.name + "/kernel"] = np.ascontiguousarray(a[:, :shp[2], :shp[3]]).reshape(shp)
            out[c.name + "/bias"] = np.ascontiguousarray(self.view(buf, c.name + "/bias").detach().float().cpu().numpy()[:shp[3] if c.kind != "up" else shp[2]])
        out["codebook/codebook"] = self.view(buf, "codebook/codebook").detach().float().cpu().numpy()
        return out

    def refresh_compute_copies(self, cast=False):
        """bf16 master copy (cast) + every derived weight layout of the step, in two batched launches: the [in,out] -> [out,in]
        transposes (forward kernels, transposed-conv dy kernels, codebook) and the tap gathers (dgrad / output-parity kernels).
        A transpose whose row count needs zero padding to the 64-multiple K pitch (none in the shipped configurations) keeps its
        own launch."""
        if cast:
            dh.cast_f32_bf16(self.p, self.pb, self.total)
        if self._refresh_tables is None:
            T = lowering.refresh_tables(self.convs, self.offset, self._wc_off, self.n_hid, self.num_tokens)
            for k in ("tr", "ga"):
                T[k] = torch.tensor(T[k], dtype=torch.int64, device=self.dev) if T[k] else None
            self._refresh_tables = T
        T = self._refresh_tables
        dh.transpose_batch(self.pb, self.wcopies, T["tr"], T["tr"].shape[0], T["tiles"])
        if T["ga"] is not None:
            dh.weight_gather_batch(self.pb, self.wcopies, T["ga"], T["ga"].shape[0], T["blocks"])
        for name, kind, R, Rp, C in T["padded"]:
            dh.transpose_padded(self.view(self.pb, name + "/kernel"), getattr(self, kind)[name], R, Rp, C)
        if self.vq_on:
            dh.vq_half_norms(self.h, self.num_tokens, self.n_hid, codebook_t=self.codebook_t, ldc=self.n_hid)

    # ------------------------------------------------------------------ conv building blocks
    def _w(self, name):
        return self.view(self.pb, name)

    _implicit_ok = staticmethod(lowering.implicit_ok)    # (bench.py and the tests ask it of a layer)

    def _gather(self, t, x, col=None):
        """the column matrix of x through t's taps: dmi_im2col into `col` (self.col when None); a direct product reads x itself"""
        if t.direct:
            return x
        col = self.col if col is None else col
        dh.im2col(x, col, self.B, t.H, t.W, t.C, t.Ho, t.Wo, t.stride, t.taps, t.Kp)
        return col

    def _tap_product(self, t, x, w, out, flags=0, col=None, **epilogue):
        """out [B*Ho*Wo, N] = (x through t's taps) . w^T: gathered inside dmi_conv_gemm_nt, or the plain dmi_gemm_nt on the column
        `col` (None: gathered into self.col now)"""
        if t.implicit:
            dh.conv_gemm_nt(x, self.B, t.H, t.W, t.C, t.Ho, t.Wo, t.stride, t.taps, w, t.Kp, out, t.N, t.N, flags, **epilogue)
            return
        col = self._gather(t, x) if col is None else col
        dh.gemm_nt(col, t.Kp, w, t.Kp, out, t.N, self.B * t.Ho * t.Wo, t.N, t.Kp, flags, **epilogue)

    def _tap_wgrad(self, t, x, dy, dW, ws, dfr, dbias=None, col=None):
        """dW [(tap, c)][N] = (x through t's taps)^T . dy, with the bias gradient when `dbias`: gathered inside dmi_conv_wgrad_tn,
        or dmi_gemm_tn on the column `col` (None: gathered into self.col now)"""
        if t.implicit:
            dh.conv_wgrad_tn(x, self.B, t.H, t.W, t.C, t.Ho, t.Wo, t.stride, t.taps, dy, t.N, t.N, dW, ws, dbias=dbias, deferred=dfr)
            return
        col = self._gather(t, x) if col is None else col
        dh.gemm_tn(col, t.Kp, dy, t.N, dW, self.B * t.Ho * t.Wo, t.K, t.N, ws, dbias=dbias, deferred=dfr)

    def _conv_fwd(self, c: _Conv, x, out, flags=0, residual=None):
        B = self.B
        bias = self._w(c.name + "/bias")
        if c.kind == "up":      # 4 output-parity GEMMs + interleave
            Mi = B * c.H * c.W
            for q, t in enumerate(c.fwd):
                self._tap_product(t, x, self.wp[c.name][q], self.par[q * Mi * c.cout:], dh.GEMM_BIAS, bias=bias)
            dh.pixel_interleave(self.par, out, B, c.H, c.W, c.cout)
            return
        t, = c.fwd
        col = None
        if self.keep_cols and c.kind != "final" and not t.implicit:     # the weight gradient of this step reads the column again
            col = self.col_keep.get(c.name)
            if col is None:
                col = self.col_keep[c.name] = torch.empty(B * t.Ho * t.Wo * t.Kp, dtype=torch.bfloat16, device=self.dev)
            self._col_valid.add(c.name)
            self._gather(t, x, col)
        hook = self.event_hook          # bench.py: HIP events around one named implicit convolution launch
        timed = hook is not None and hook[0] == c.name and t.implicit
        if timed:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        self._tap_product(t, x, self.wf[c.name], out, flags | dh.GEMM_BIAS, col=col, bias=bias, residual=residual)
        if timed:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            hook[1].append((e0, e1))

    # ------------------------------------------------------------------ forward
    def _units(self, lo, hi):
        """convs[lo:hi] as the units every pass walks: (i, layer, None) for a down / up / final layer on its own, (i, conv_in,
        conv_out) for the residual pair at i, i + 1"""
        i = lo
        while i < hi:
            c = self.convs[i]
            pair = c.kind == "res"
            yield i, c, self.convs[i + 1] if pair else None
            i += 2 if pair else 1

    def _run_layers(self, lo, hi, x):
        """forward of convs[lo:hi] from x: fills act_in / act_out and returns the last output"""
        for i, c, c_out in self._units(lo, hi):
            self.act_in[i] = x
            if c_out is None:
                self._conv_fwd(c, x, self.act_out[i])
                x = self.act_out[i]
            else:  # residual pair: conv_in (bias+relu), conv_out (bias + residual x)
                self._conv_fwd(c, x, self.act_out[i], flags=dh.GEMM_RELU)
                self.act_in[i + 1] = self.act_out[i]
                self._conv_fwd(c_out, self.act_out[i], self.act_out[i + 1], flags=dh.GEMM_RESIDUAL, residual=x)
                x = self.act_out[i + 1]
        return x

    def forward(self, features, return_recon_loss=False, return_logits=False, hard_gumbel=True, temperature=1.0, noise=None,
                need_grad=None):
        """features: images NHWC fp32 in [-1,1] (or {"inputs": ...}).  Mirrors vae_tf/models.py:165-184.
        `noise`: optional uniforms [B,g,g,num_tokens] in [1e-9,1) (injected for parity; drawn with torch.rand otherwise)."""
        img = features["inputs"] if isinstance(features, dict) else features
        img = img.to(device=self.dev, dtype=torch.float32).contiguous()
        B = self.B
        assert img.shape == (B, self.H, self.W, self.num_ch), f"expected {(B, self.H, self.W, self.num_ch)}, got {tuple(img.shape)}"
        self.img = img
        if return_logits and self.fp32_tokens:
            return self.encode_logits_fp32(img)
        self._col_valid.clear()
        Np = B * self.Hs * self.Hs
        if self.stack_factor > 1:
            dh.space_to_depth_f32(img, self.img_st, B, self.Hs, self.Hs, self.num_ch, self.stack_factor, self.c_st)
            img = self.img_st          # the loss is permutation-invariant: computed in the stacked layout
        self.img_net = img
        dh.pad_channels(img, self.x_img, Np, self.c_st, self.img_cp)
        x = self._run_layers(0, self.n_enc, self.x_img)
        self.x_enc = x
        if self.vq_on:
            return self._forward_vq(return_recon_loss, return_logits, need_grad)
        dh.gemm_nt(x, self.n_hid, self.codebook_t, self.n_hid, self.logits, self.num_tokens, self.Mg, self.num_tokens, self.n_hid,
                   dh.GEMM_OUT_F32)
        self._kl_fresh = False
        if return_logits:
            return self.logits.view(B, self.grid, self.grid, self.num_tokens)
        kl_on = self.kl_weight > 0 and return_recon_loss
        if kl_on:
            dh.codebook_kl_fwd(self.logits, self.rowstat, self.loss_kl, self.Mg, self.num_tokens, self.ws_kl)
            self._kl_fresh = True
        if noise is None:
            self.u.uniform_(1e-9, 1.0)
        elif not (isinstance(noise, str) and noise == "preset"):   # "preset": self.u was filled by the caller (graph replay)
            self.u.copy_(noise.to(self.dev).reshape(self.Mg, self.num_tokens))
        self.temperature = float(temperature)
        dh.gumbel_softmax_fwd(self.logits, self.u, self.y, self.y_soft, self.index, self.Mg, self.num_tokens, self.temperature,
                              hard_gumbel, temperature_dev=self._temp_dev())
        x = self._decoder_from_y()
        if not return_recon_loss:
            return self.reconstruction()
        need_grad = (self.mode == "train") if need_grad is None else need_grad
        # d(out) of mean((img-out)^2); 1/world folds the CrossShardOptimizer mean (src/model_fns_tf.py:61) into the gradient
        dh.mse_loss(self.img_net, x, self.ga if need_grad else None, self.loss_recon if kl_on else self.loss, B * self.Hs * self.Hs,
                    self.c_st, OUT_CP, 1.0, self.ws)
        if kl_on:       # loss = recon + beta_t KL on the device; beta_t by value, or from _dyn on the graph path
            if not self._dyn_on:
                self.kl_weight_t = kl_weight_at(self.global_step, self.kl_weight, self.kl_anneal_steps)
            dh.elbo_loss(self.loss_recon, self.loss_kl, self.loss, self.kl_weight_t, kl_weight_dev=self._kl_dev())
        return self.loss[0], self.reconstruction()

    def _forward_vq(self, return_recon_loss, return_logits, need_grad):
        """the rest of forward() under "quantizer": "vq": dmi_vq_assign (index, and xq straight into the decoder's input), decoder,
        dmi_mse_loss, dmi_vq_loss, loss = recon + (1 + beta) Lq.  return_logits: the scores s = x . C - h as [B, g, g, T] fp32, whose
        arg-max is the code (the logits product, then dmi_vq_scores_bias)"""
        B, T, nh, Mg = self.B, self.num_tokens, self.n_hid, self.Mg
        if return_logits:
            self._logits_buffer()
            dh.gemm_nt(self.x_enc, nh, self.codebook_t, nh, self.logits, T, Mg, T, nh, dh.GEMM_OUT_F32)
            dh.vq_scores_bias(self.logits, self.h, Mg, T)
            return self.logits.view(B, self.grid, self.grid, T)
        dh.vq_assign(self.x_enc, nh, self.codebook_t, nh, self.h, self.index, self.xdec, nh, None, Mg, T, nh)
        x = self._decoder_from_xdec()
        if not return_recon_loss:
            return self.reconstruction()
        need_grad = (self.mode == "train") if need_grad is None else need_grad
        dh.mse_loss(self.img_net, x, self.ga if need_grad else None, self.loss_recon, B * self.Hs * self.Hs, self.c_st, OUT_CP, 1.0, self.ws)
        dh.vq_loss(self.x_enc, nh, self.xdec, nh, self.loss_vq, Mg, nh, self.ws_vq)
        # the EMA codebook has no codebook loss: commitment only
        dh.elbo_loss(self.loss_recon, self.loss_vq, self.loss, self.vq_beta if self.vq_ema is not None else 1.0 + self.vq_beta)
        return self.loss[0], self.reconstruction()

    def _logits_buffer(self):
        if self.logits is None:
            self.logits = torch.empty(self.Mg, self.num_tokens, dtype=torch.float32, device=self.dev)

    def _decoder_from_y(self):
        """decoder (vae_tf/models.py:123-163) on self.y [Mg, num_tokens] (soft / hard one-hot): y @ codebook^T, then per reversed
        block a 4x4 s2 conv-transpose and the residual stacks, final 1x1 conv -> self.out_pad"""
        dh.gemm_nt(self.y, self.num_tokens, self._w("codebook/codebook"), self.num_tokens, self.xdec, self.n_hid, self.Mg, self.n_hid,
                   self.num_tokens)
        return self._decoder_from_xdec()

    def _decoder_from_xdec(self):
        """the decoder's convolutions on self.xdec [Mg, n_hid] -> self.out_pad"""
        x = self._run_layers(self.n_enc, len(self.convs), self.xdec)
        self.out_pad = x
        return x

    def decode_tokens(self, tokens):
        """image-token ids [B, g*g] (what DALL-E emits) -> images [B,H,W,C] fp32: one-hot rows through the decoder.
        The sampling half the reference leaves unfinished (predict raises upstream, src/model_fns.py:135-136)."""
        tok = tokens.to(device=self.dev, dtype=torch.int64).reshape(self.Mg)
        assert int(tok.min()) >= 0 and int(tok.max()) < self.num_tokens
        if self.vq_on:       # the code itself: rows of codebook_t by index
            dh.vq_gather(self.codebook_t, self.n_hid, tok.to(torch.int32), self.xdec, self.n_hid, self.Mg, self.num_tokens, self.n_hid)
            self._decoder_from_xdec()
            return self.reconstruction()
        self.y.zero_()
        self.y.scatter_(1, tok.view(-1, 1), 1.0)       # index plumbing: the one-hot the hard Gumbel path would produce
        self._decoder_from_y()
        return self.reconstruction()

    def reconstruction(self):
        out = torch.empty(self.B, self.H, self.W, self.num_ch, dtype=torch.float32, device=self.dev)
        if self.stack_factor == 1:
            dh.unpad_channels(self.out_pad, out, self.B * self.H * self.W, self.num_ch, OUT_CP)
            return out
        st = torch.empty(self.B * self.Hs * self.Hs, self.c_st, dtype=torch.float32, device=self.dev)
        dh.unpad_channels(self.out_pad, st, self.B * self.Hs * self.Hs, self.c_st, OUT_CP)
        dh.depth_to_space_f32(st, out, self.B, self.Hs, self.Hs, self.num_ch, self.stack_factor, self.c_st)
        return out

    # ------------------------------------------------------------------ fp32 tokenising encoder
    def encode_logits_fp32(self, img):
        """Encoder + `x @ codebook` entirely in fp32 from the fp32 master weights (dmi_conv2d_f32): the path the reference
        takes when the VAE tokenises images for DALL-E (src/model_fns.py:43-51 builds it without use_bf16; encoder
        src/vae_tf/models.py:81-120).  Forward only.  Returns logits [B, g, g, num_tokens] fp32."""
        B, dev = self.B, self.dev
        if self._f32 is None:
            mx = max(B * c.Ho * c.Wo * c.cout for c in self.convs[:self.n_enc])
            self._f32 = dict(x=torch.empty(B * self.Hs * self.Hs, self.img_cp, dtype=torch.float32, device=dev),
                             a=[torch.empty(mx, dtype=torch.float32, device=dev) for _ in range(3)])
        f = self._f32
        self._logits_buffer()
        dh.space_to_depth_f32(img, f["x"], B, self.Hs, self.Hs, self.num_ch, self.stack_factor, self.img_cp)
        x, free = f["x"], list(f["a"])

        def conv(c, xin, out, relu=False, residual=None):
            t, = c.fwd
            dh.conv2d_f32(xin, B, t.H, t.W, t.C, t.Ho, t.Wo, t.stride, t.taps, self.view(self.p, c.name + "/kernel"),
                          self.view(self.p, c.name + "/bias"), residual, out, c.cout, relu=relu)
        for _, c, c_out in self._units(0, self.n_enc):
            if c_out is None:
                out = free.pop(0)
                conv(c, x, out)
                if x is not f["x"]:
                    free.append(x)
            else:
                h, out = free.pop(0), free.pop(0)
                conv(c, x, h, relu=True)
                conv(c_out, h, out, residual=x)
                free.extend([h, x])
            x = out
        if self.vq_on:
            self.x_enc_f32 = x   # fp32 [Mg, n_hid] at the front of one of the path's scratch buffers, until its next call (read by the tests)
        dh.conv2d_f32(x, self.Mg, 1, 1, self.n_hid, 1, 1, 1, [(0, 0)], self.view(self.p, "codebook/codebook"), None, None,
                      self.logits, self.num_tokens)
        if self.vq_on:       # s = x . C - h, both from the fp32 masters
            if self.h32 is None:
                self.h32 = torch.empty(self.num_tokens, dtype=torch.float32, device=dev)
            dh.vq_half_norms(self.h32, self.num_tokens, self.n_hid, codebook_f32=self.view(self.p, "codebook/codebook"))
            dh.vq_scores_bias(self.logits, self.h32, self.Mg, self.num_tokens)
        self._kl_fresh = False
        return self.logits.view(B, self.grid, self.grid, self.num_tokens)

    # ------------------------------------------------------------------ backward
    def _gv(self, name):
        return self.view(self.g, name)

    def _defer_ws(self, defer):
        """(workspace, deferred list or None) of the next weight gradient: immediate reduce on the shared workspace, or a pool
        slot whose reduces run at the next _flush_reduces()"""
        if not defer:
            return self.ws, None
        if self._ws_next >= WS_POOL:
            self._flush_reduces()
        w = self.ws_pool[self._ws_next]
        self._ws_next += 1
        return w, self.deferred

    def _flush_reduces(self):
        self.deferred.run()
        self._ws_next = 0

    def _wgrad(self, c: _Conv, x_in, dy, defer=False):
        """dW[(k,ci)][co] = col(x)^T . dy (+ bias gradient fused) -- lands directly in the TF kernel layout."""
        ws, dfr = self._defer_ws(defer)
        col = self.col_keep[c.name] if c.name in self._col_valid else None    # the forward pass of this step kept col(x_in)
        self._tap_wgrad(c.wgrad, x_in, dy, self._gv(c.name + "/kernel"), ws, dfr, dbias=self._gv(c.name + "/bias"), col=col)

    def _dgrad3(self, c: _Conv, dy, out, flags=0, residual=None, relu_src=None):
        self._tap_product(c.dgrad[0], dy, self.wd[c.name], out, flags, residual=residual, relu_src=relu_src)

    def _up_backward(self, c: _Conv, x_in, dz, out, defer=False):
        """backward of the transposed conv z = conv2d_transpose(y) (vae_tf/models.py:133-137): a stride-2 4x4 SAME conv of dz.
        dW[kh,kw,Cout,Cin] and dbias into g, dy [B*H*W, cin] into `out`.  Both products read one gather of dz."""
        t = c.wgrad
        ws, dfr = self._defer_ws(defer)
        col = None if t.implicit else self._gather(t, dz)       # stride-2 conv view of dz
        dh.colsum(dz, c.cout, self._gv(c.name + "/bias"), self.B * c.Ho * c.Wo, c.cout, self.ws_cs)
        self._tap_wgrad(t, dz, x_in, self._gv(c.name + "/kernel"), ws, dfr, col=col)
        self._tap_product(t, dz, self.wd[c.name], out, col=col)

    def _dgrad_down(self, c: _Conv, dy, out):
        """input gradient of the 4x4 stride-2 SAME conv (vae_tf/models.py:90-92) = its transposed conv: 4 output-parity GEMMs
        over the 2x2 contributing taps + a pixel interleave; dy [B*Ho*Wo, cout] -> out [B*H*W, cin]."""
        Mo = self.B * c.Ho * c.Wo
        for q, t in enumerate(c.dgrad):
            self._tap_product(t, dy, self.wp[c.name][q], self.par[q * Mo * c.cin:], 0)
        dh.pixel_interleave(self.par, out, self.B, c.Ho, c.Wo, c.cin)

    def backward(self):
        """Gradients of the last forward(return_recon_loss=True) into the flat fp32 buffer `g`."""
        B = self.B
        d = self.ga                       # gradient wrt the padded reconstruction [M0, 64]
        spare = [self.gb, self.gc]
        mark = [self.total]               # g[mark, total) has been handed to the exchange

        def ready_down_to(off):           # the layout follows the forward order, backward finishes it from the end
            if off < mark[0]:
                if self.world > 1:
                    self._flush_reduces()  # the exchange takes g[off, mark): its pending slab reduces must have landed
                self.reducer.ready(off, mark[0])
                mark[0] = off
        for i, c, c_out in reversed(list(self._units(0, len(self.convs)))):     # (a residual pair is processed as one unit)
            if c.kind == "final":
                M = B * c.H * c.W
                self._wgrad(c, self.act_in[i], d, defer=True)
                nd = spare[0]
                dh.gemm_nt(d, c.cout, self._w(c.name + "/kernel"), c.cout, nd, c.cin, M, c.cin, c.cout)   # K = 64 padded channels
                spare[0], d = d, nd
            elif c_out is not None:         # residual pair: c = conv_in at i, c_out = conv_out at i + 1
                x_in, r = self.act_in[i], self.act_in[i + 1]
                if self.recompute_grad:      # re-run the branch's first conv into the shared buffer (bit-identical to the forward)
                    self._conv_fwd(c, x_in, r, flags=dh.GEMM_RELU)
                self._wgrad(c_out, r, d, defer=True)
                da = spare[0]
                self._dgrad3(c_out, d, da, flags=dh.GEMM_RELU_MASK, relu_src=r)
                self._wgrad(c, x_in, da, defer=True)
                nd = spare[1]
                self._dgrad3(c, da, nd, flags=dh.GEMM_RESIDUAL, residual=d)
                spare[1], d = d, nd
            elif c.kind == "up":
                nd = spare[0]
                self._up_backward(c, self.act_in[i], d, nd, defer=True)
                spare[0], d = d, nd
            else:  # down
                self._wgrad(c, self.act_in[i], d, defer=True)
                if i > 0:
                    nd = spare[0]
                    self._dgrad_down(c, d, nd)
                    spare[0], d = d, nd
            ready_down_to(self.offset[c.name + "/kernel"])
            if i == self.n_enc and self.vq_on:
                # ---- VQ bottleneck: straight-through d plus the commitment gradient to the encoder, the codebook loss to the codebook
                T, nh, Mg = self.num_tokens, self.n_hid, self.Mg
                nd = spare[0]
                dh.vq_bwd_x(d, nh, self.x_enc, nh, self.xdec, nh, nd, nh, Mg, nh, self.vq_beta)
                if self.vq_ema is None:      # (EMA codebook: no gradient; its slice of g keeps the zeros it was allocated with)
                    dh.vq_codebook_grad(self.x_enc, nh, self.index, self.codebook_t, nh, self._gv("codebook/codebook"), Mg, T, nh, self.ws_vq)
                spare[0], d = d, nd
                ready_down_to(self.offset["codebook/codebook"])
            elif i == self.n_enc:
                # ---- tied codebook + gumbel (between decoder and encoder); d = gradient wrt xdec [Mg, n_hid]
                T, nh, Mg = self.num_tokens, self.n_hid, self.Mg
                dh.gemm_tn(d, nh, self.y, T, self.gc2, Mg, nh, T, self.ws)                               # dC from x_dec = y C^T
                dh.gemm_nt(d, nh, self.codebook_t, nh, self.dy, T, Mg, T, nh)                            # dy = dxdec . C
                if self.kl_weight > 0:     # the KL gradient (beta_t / M) q (ln q - e) joins before the one bf16 rounding
                    dh.gumbel_softmax_bwd_kl(self.dy, self.y_soft, self.logits, self.rowstat, self.dlogits, Mg, T, self.temperature,
                                             self.kl_weight_t, temperature_dev=self._temp_dev(), kl_weight_dev=self._kl_dev())
                else:
                    dh.gumbel_softmax_bwd(self.dy, self.y_soft, self.dlogits, Mg, T, self.temperature, temperature_dev=self._temp_dev())
                dh.gemm_tn(self.x_enc, nh, self.dlogits, T, self._gv("codebook/codebook"), Mg, nh, T, self.ws)  # dC from logits = x C
                dh.add_f32(self._gv("codebook/codebook"), self.gc2, nh * T)
                nd = spare[0]
                dh.gemm_nt(self.dlogits, T, self._w("codebook/codebook"), T, nd, nh, Mg, nh, T)          # dx_enc = dlogits . C^T
                spare[0], d = d, nd
                ready_down_to(self.offset["codebook/codebook"])
        ready_down_to(0)
        self._flush_reduces()

    # ------------------------------------------------------------------ optimizer
    def optimizer_step(self, lr, beta1=0.9, beta2=0.999, eps=1e-8):
        """tf.train.AdamOptimizer (src/model_fns_tf.py:58-60; Appendix A.8): lr_t = lr*sqrt(1-b2^t)/(1-b1^t);
        p -= lr_t*m/(sqrt(v)+eps).  grad_scale 1/world = CrossShardOptimizer's mean over replicas (:61)."""
        self.reducer.finish()
        lr_t = self.lr_t(lr, beta1, beta2)
        dh.adam_step(self.p, self.g, self.m, self.v, self.pb, self.total, None, 0.0, lr_t, beta1, beta2, eps, 0.0, 1.0 / self.world,
                     lr_dev=self._dyn[0:1] if self._dyn_on else None)
        if self.vq_ema is not None:
            self._ema_codebook_step()
        self.refresh_compute_copies(cast=False)
        self.global_step += 1

    def _ema_codebook_step(self):
        """the codebook's own update (Adam left it alone: its gradient is 0): cluster sums of this step's x_enc / index, the moving
        averages, the restarts; into the fp32 master and its bf16 copy, between dmi_adam_step and refresh_compute_copies"""
        e, T, nh, Mg = self.vq_ema, self.num_tokens, self.n_hid, self.Mg
        dh.vq_cluster_sums(self.x_enc, nh, self.index, self._ema_sums, self._ema_counts, Mg, T, nh, self._ema_ws)
        dh.vq_ema_step(self.view(self.p, "codebook/codebook"), self.view(self.pb, "codebook/codebook"), e["N"], e["S"], e["idle"],
                       e["restarts"], self._ema_sums, self._ema_counts, self.x_enc, nh, self.vq_ema_decay, self.vq_restart_after,
                       self.vq_restart_seed, self.global_step, Mg, T, nh, step_dev=self._step_dev if self._dyn_on else None)

    def lr_t(self, lr, beta1=0.9, beta2=0.999):
        t = self.global_step + 1
        return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)

    # ------------------------------------------------------------------ whole step as one HIP graph
    def _temp_dev(self):
        return self._dyn[1:2] if self._dyn_on else None

    def _kl_dev(self):
        return self._dyn[2:3] if self._dyn_on else None

    def train_step(self, features, lr, hard_gumbel=True, temperature=1.0, noise=None, graph=None):
        """forward + backward + optimizer_step.  The small configurations are launch-bound (vae_example: ~170 launches of a
        few microseconds each; 3.2 ms per step from Python against ~1 ms of kernel time, profiles/r02_bench_vae_example.json),
        so the step is captured ONCE as a HIP graph and replayed: per step the host then issues the image copy, the Gumbel
        uniforms (drawn eagerly), two scalar fills and one graph launch.  The learning rate lr_t
        (tf.train.AdamOptimizer's bias-corrected rate, src/model_fns_tf.py:58) and the annealed temperature (:40-45) live in
        a small device buffer the kernels read (dmi_adam_step lr_dev / dmi_gumbel_softmax_* temperature_dev), and with
        kl_loss_weight > 0 so does the ramped KL weight beta_t (dmi_gumbel_softmax_bwd_kl / dmi_elbo_loss kl_weight_dev), so one
        graph serves the whole schedule.  Eager when: data-parallel (the exchange runs on its own stream and communicator), a
        bench event hook is set, DALLE_VAE_GRAPH=0, or graph=False.  Same kernels, same order: results are bit-identical to
        the eager step (tested).  Returns the device scalar loss."""
        want = (os.environ.get("DALLE_VAE_GRAPH", "1") != "0") if graph is None else bool(graph)
        img = features["inputs"] if isinstance(features, dict) else features
        if not want or self.world > 1 or self.event_hook is not None:
            self.forward(img, return_recon_loss=True, hard_gumbel=hard_gumbel, temperature=temperature, noise=noise, need_grad=True)
            self.backward()
            self.optimizer_step(lr)
            return self.loss[0]
        if self._img_static is None:
            self._img_static = torch.empty(self.B, self.H, self.W, self.num_ch, dtype=torch.float32, device=self.dev)
        self._img_static.copy_(img.to(dtype=torch.float32), non_blocking=True)
        if self.vq_on:
            hard_gumbel = True       # accepted and ignored: one graph
        elif noise is None:
            self.u.uniform_(1e-9, 1.0)
        else:
            self.u.copy_(noise.to(self.dev).reshape(self.Mg, self.num_tokens))
        self._dyn[0:1].fill_(self.lr_t(lr))          # by-value kernel arguments: no host buffer whose lifetime could race a replay
        self._dyn[1:2].fill_(float(temperature))
        if self.kl_weight > 0:
            self.kl_weight_t = kl_weight_at(self.global_step, self.kl_weight, self.kl_anneal_steps)
            self._dyn[2:3].fill_(self.kl_weight_t)
        if self.vq_ema is not None:
            self._step_dev.fill_(self.global_step)       # the restart hash's step, as lr_t is: one graph serves every step
        self.temperature = float(temperature)
        key = bool(hard_gumbel)
        g = self._graphs.get(key)
        if g is None:
            self._dyn_on = True
            try:
                if not self._graph_warm:
                    # first step eager (on the kernels' device-scalar path): lazily allocated buffers come into being
                    # outside the capture
                    self._step_body(key)
                    self._graph_warm = True
                    return self.loss[0]      # (forward() ran in Python: _kl_fresh is as it left it)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                step0 = self.global_step
                with torch.cuda.graph(g, capture_error_mode="thread_local"):   # other host threads (input producer) stay free to call HIP
                    self._step_body(key)
                self.global_step = step0          # capture records, it does not execute: the replay below is the step
                self._graphs[key] = g
            finally:
                self._dyn_on = False
        g.replay()
        self.global_step += 1
        self._kl_fresh = self.kl_weight > 0     # the replay rewrote logits; it ran dmi_codebook_kl_fwd on them only with a KL weight
        return self.loss[0]

    def _step_body(self, hard_gumbel):
        self.forward(self._img_static, return_recon_loss=True, hard_gumbel=hard_gumbel, temperature=1.0, noise="preset", need_grad=True)
        self.backward()
        self.optimizer_step(1.0)      # lr / temperature arguments are ignored on the device-scalar path

    # ------------------------------------------------------------------ codebook statistics
    def codebook_stats(self):
        """Codebook health on the last forward's logits / index (outside the captured step; call it where something is logged):
        kl = mean over positions of KL(q || uniform) in nats, perplexity_soft = exp(H(mean_m q[m, :])), perplexity_hard =
        exp(H(counts / M)) of the codes the Gumbel arg-max picked, codes_used = #{counts > 0} and codes_used_frac = codes_used /
        num_tokens.  dmi_codebook_kl_fwd (unless the forward ran it) and dmi_codebook_usage; the two entropies over [num_tokens]
        are taken on the host in float64.  One device-to-host copy."""
        T, Mg = self.num_tokens, self.Mg
        if self.vq_on:       # the picks alone: there is no posterior, so no kl and no perplexity_soft
            if self._usage is None:
                self._usage = dict(counts=torch.empty(T, dtype=torch.int32, device=self.dev))
                self.ws_kl = torch.empty(int(dh.codebook_kl_workspace_bytes(Mg, T)) + 1024, dtype=torch.uint8, device=self.dev)
            dh.codebook_usage(None, None, self.index, None, self._usage["counts"], Mg, T, self.ws_kl)
            counts = self._usage["counts"].cpu().numpy()
            used = int((counts > 0).sum())
            out = dict(perplexity_hard=_perplexity(counts), codes_used=used, codes_used_frac=used / T)
            if self.vq_ema is not None:
                out.update(vq_restarts=int(self.vq_ema["restarts"][0]), codes_idle=int((self.vq_ema["idle"] >= 1).sum()))
            return out
        self._kl_buffers()
        if self._usage is None:
            self._usage = dict(qsum=torch.empty(T, dtype=torch.float32, device=self.dev),
                               counts=torch.empty(T, dtype=torch.int32, device=self.dev))
        u = self._usage
        if not self._kl_fresh:
            dh.codebook_kl_fwd(self.logits, self.rowstat, self.loss_kl, Mg, T, self.ws_kl)
            self._kl_fresh = True
        dh.codebook_usage(self.logits, self.rowstat, self.index, u["qsum"], u["counts"], Mg, T, self.ws_kl)
        out = dict(kl=float(self.loss_kl[0]))
        out.update(usage_stats(u["qsum"].cpu().numpy(), u["counts"].cpu().numpy(), Mg))
        return out

    def state_dict(self):
        # reference-named variables as plain tensors in a plain dict: loadable with torch.load(weights_only=True)
        sd = {"vae_variables": {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in self.export_reference().items()},
              "m": self.m.detach().cpu(), "v": self.v.detach().cpu(), "global_step": self.global_step}
        if self.vq_on:       # only when on: a checkpoint without the key is a Gumbel one
            sd["quantizer"] = "vq"
        ema = getattr(self, "vq_ema", None)     # (getattr: tests/test_vae_vq.py calls these two on a stand-in without EMA attributes)
        if ema is not None:  # likewise: a VQ checkpoint without these was trained by the codebook gradient
            sd["vq_codebook"] = "ema"
            sd["vq_ema"] = {k: ema[k].detach().cpu() for k in VQ_EMA_STATE_KEYS}
        return sd

    def load_state_dict(self, sd):
        check_checkpoint(self.quantizer, sd)
        ema = getattr(self, "vq_ema", None)
        check_ema_checkpoint(getattr(self, "vq_ema_decay", None), sd)
        self.load_reference_params({k: (v.numpy() if torch.is_tensor(v) else np.asarray(v))
                                    for k, v in sd["vae_variables"].items()})
        if "m" in sd:
            self.m.copy_(sd["m"]); self.v.copy_(sd["v"])
        if ema is not None:
            for k in VQ_EMA_STATE_KEYS:
                ema[k].copy_(torch.as_tensor(sd["vq_ema"][k]).reshape(ema[k].shape))
        self.global_step = int(sd.get("global_step", 0))
