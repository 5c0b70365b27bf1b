"""DalleEngine -- sequences the HIP kernels of libdalle_hip into the DALL-E train step.

Replaces, for the hot path, what the reference obtains from Mesh-TensorFlow's graph + lowering
(src/model_fns.py:80-94,168-202 -> mtf.Graph / mtf.Lowering) and its optimizer
(src/optimizers.py:19-104): forward (src/dalle_mtf/models.py:397-416), a hand-written backward,
global-norm clip + Adam without bias correction, and the data-parallel gradient all-reduce that mtf
inserts implicitly for `layout: batch_dim:data` -- here RCCL via
torch.distributed, bucketed and overlapped with backward on the collective's own stream.

PyTorch is plumbing only (device memory, streams, torch.distributed); all arithmetic runs in the
hand-written kernels behind the C ABI.  There is no CPU fallback.

Memory plan (HBM, per GPU): parameters live in ONE flat fp32 buffer (+ flat grads, Adam m, v -- or Adafactor's m and
factored second moments, DESIGN.md §4 "Adafactor") laid out in
reverse-usage order [to_logits | layer_{L-1} .. layer_0 | wpe | wte] so finished gradients always form
a contiguous prefix (= all-reduce buckets).  bf16 compute copies: `pb` (same offsets, natural [in,out]
layout, written by the Adam kernel) and `pbt` ([out,in] copies of the GEMM weights for the forward).
Activations needed by backward are kept in bf16 per layer (no recompute; 288 GB HBM).
"""
from __future__ import annotations

import contextlib
import gc
import hashlib
import logging
import math
import os
from collections import OrderedDict, namedtuple
from typing import Dict, Optional, Tuple

import numpy as np
import torch

import dalle_hip as dh
from ..dp import GradReducer
from .dropout import SITE_POSITION, SITE_TOKEN, site_attention, site_key, site_mlp
from .layout import ALIGN, ParamLayout, _round_up, adafactor_factored_dims, adafactor_table, reference_init   # noqa: F401  (re-exported)
from .qk_norm import GAIN_NAMES
from .kv_cache import DEFAULT as KV_DEFAULT, resolve_kv_cache_dtype
from .ema import ema_decay_at, one_minus_decay, resolve_weights   # noqa: F401  (ema_decay_at: part of the engine's surface)
from .loss_mask import mask_coefficients, resolve_loss_ignore_padding
from .loss_weights import position_weights
from .options import check_checkpoint, checkpoint_entries, resolve_options
from .rotary import rotary_table
from .token_shift import grid_side

@contextlib.contextmanager
def _no_gc_in_capture():
    """For the span of a stream capture: collect garbage first, then keep the cyclic collector off.  torch.cuda.graph no longer
    collects before it captures, and a collection that starts inside the capture runs finalisers there -- a dead model's
    CUDAGraph among them, whose destruction synchronises the device, a call the capturing thread may not make: the runtime
    reports it from a destructor and the process aborts.  Collecting first also finalises such objects where that is legal."""
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_enabled:
            gc.enable()


HEAD_DIMS = (64, 128)   # n_embd / n_heads values the attention kernels are built for
# the variant of the sampler's draw: the plain, the nucleus (with or without the log-likelihood) or the guided kernel, which is a
# nucleus one.  Keys the captured decode graphs; False there is the decode_step body, which draws nothing
Draw = namedtuple("Draw", "nucleus guided logp")


def draw_params(v, temperature, top_k, seed, top_p, guidance_scale):
    """the device parameter block of variant v (a Draw): four words for the plain draw, six for the others (dalle_hip.sample_params)"""
    return dh.sample_params(temperature, top_k, seed, top_p if v.nucleus else None, guidance_scale if v.guided else None)


SampleArgs = namedtuple("SampleArgs", "rows guided guidance_scale top_p uncond_text image_prefix prefix_len")


def check_sample_args(B, T, P, text_vocab_size, image_vocab_size, text, top_p=1.0, guidance_scale=1.0, uncond_text=None,
                      image_prefix=None, padding_id=None):
    """the argument checks of DalleEngine.sample_image_tokens for an engine of B rows, T text and P image positions; needs no
    device.  Returns SampleArgs: rows = the rows of text / image_prefix / the result (B, or B / 2 under guidance), uncond_text
    (guided: given or the null caption, T copies of padding_id, or of text_vocab_size - 1 when that is None) and image_prefix as
    tensors, prefix_len = k."""
    gs = float(guidance_scale)
    if not (gs >= 0.0 and math.isfinite(gs)):
        raise ValueError(f"sample_image_tokens: guidance_scale must be finite and >= 0 (got {guidance_scale})")
    guided = gs != 1.0 or uncond_text is not None
    R = B
    if guided:
        if B % 2:
            raise ValueError(f"sample_image_tokens: guidance pairs the engine's rows, so its batch must be even (B = {B})")
        R = B // 2
        if tuple(text.shape) != (R, T):
            raise ValueError(f"sample_image_tokens: with guidance text must be [B / 2 = {R}, T = {T}] (got {tuple(text.shape)})")
        if uncond_text is None:
            uncond_text = torch.full((T,), text_vocab_size - 1 if padding_id is None else int(padding_id), dtype=torch.int32)
        uncond_text = torch.as_tensor(uncond_text)
        if uncond_text.dtype.is_floating_point or uncond_text.dtype == torch.bool:
            raise ValueError("sample_image_tokens: uncond_text must hold integer token ids")
        if tuple(uncond_text.shape) not in ((T,), (R, T)):
            raise ValueError(f"sample_image_tokens: uncond_text must be [T = {T}] or [B / 2 = {R}, T = {T}] "
                             f"(got {tuple(uncond_text.shape)})")
        if int(uncond_text.min()) < 0 or int(uncond_text.max()) >= text_vocab_size:
            raise ValueError(f"sample_image_tokens: uncond_text ids must lie in [0, {text_vocab_size})")
    assert text.shape == (R, T)
    top_p = float(top_p)
    if not (0.0 < top_p <= 1.0):
        raise ValueError(f"sample_image_tokens: top_p must lie in (0, 1] (got {top_p})")
    k = 0
    if image_prefix is not None:
        image_prefix = torch.as_tensor(image_prefix)
        if image_prefix.dim() != 2 or image_prefix.shape[0] != R or not (0 <= image_prefix.shape[1] < P):
            raise ValueError(f"sample_image_tokens: image_prefix must be [B={R}, k] with 0 <= k < {P} (got {tuple(image_prefix.shape)})")
        if image_prefix.dtype.is_floating_point or image_prefix.dtype == torch.bool:
            raise ValueError("sample_image_tokens: image_prefix must hold integer token ids")
        k = int(image_prefix.shape[1])
        if k and (int(image_prefix.min()) < 0 or int(image_prefix.max()) >= image_vocab_size):
            raise ValueError(f"sample_image_tokens: image_prefix ids must lie in [0, {image_vocab_size})")
    return SampleArgs(R, guided, gs, top_p, uncond_text if guided else None, image_prefix, k)


class DalleEngine:
    def __init__(self, n_embd, n_layers, n_heads, text_vocab_size, image_vocab_size, text_seq_len, image_seq_len,
                 batch_size, global_batch_size=None, eos_token_id=None, hparams: Optional[dict] = None,
                 device="cuda", process_group=None, world_size=1, comm=None, attn_masks=None):
        self.hp = dict(hparams or {})
        # the options of hparams, resolved ahead of any device work (an activation_fn that is unset or empty is the reference's "relu"),
        # and read as the engine's own attributes: dalle_mtf.options.Options names them and says what each is
        self.options = resolve_options(self.hp, n_embd, text_seq_len, image_seq_len, activation_fn=self.hp.get("activation_fn") or "relu")
        for name, value in self.options._asdict().items():
            setattr(self, name, value)
        # hparams["loss_ignore_padding"] (dalle_mtf.loss_mask): a training setting beside the options, like the sampler's cache type
        self.loss_ignore_padding, self.loss_pad_id = resolve_loss_ignore_padding(self.hp, text_seq_len, text_vocab_size)
        if not torch.cuda.is_available():
            raise dh.DalleHipError("DalleEngine needs a HIP device (MI355X); there is no CPU fallback")
        dh.lib()
        assert n_embd % n_heads == 0, "n_state must be divisible by n_heads"
        if n_embd // n_heads not in HEAD_DIMS:
            raise dh.DalleHipError(f"attention kernels are built for head dims 64 and 128 (n_embd/n_heads = {n_embd // n_heads}); "
                                   "the reference README recommends 128")
        self.d, self.L, self.H = n_embd, n_layers, n_heads
        self.hd = n_embd // n_heads   # selects the attention kernels
        self.text_vocab_size, self.image_vocab_size = text_vocab_size, image_vocab_size
        self.T, self.S = text_seq_len, text_seq_len + image_seq_len
        assert self.S % 8 == 0, "total sequence length must be a multiple of 8"
        self.V = text_vocab_size + image_vocab_size + 1
        self.eos = self.V - 1 if eos_token_id is None else eos_token_id
        self.B = batch_size
        self.B_global = global_batch_size or batch_size * world_size
        self.M = self.B * self.S
        self.dev = torch.device(device)
        self.pg, self.world = process_group, world_size
        self.lay = ParamLayout(n_embd, n_layers, n_heads, self.V, self.S, ff_glu=self.ff_glu, qk_norm=self.qk_norm)
        self.F1 = self.lay.ffn1      # FFN-1's output width: 4d, gated [value | gate] = 8d
        self.Vp = self.lay.Vp
        n = self.lay.total
        f32 = dict(dtype=torch.float32, device=self.dev)
        b16 = dict(dtype=torch.bfloat16, device=self.dev)
        self.p = torch.zeros(n, **f32)
        self.g = torch.zeros(n, **f32)
        self.optimizer = None
        self.set_optimizer(self.hp.get("optimizer") or "adam")
        self.pb = torch.zeros(n, **b16)
        self.pbt = torch.zeros(self.lay.t_total, **b16)
        # hparams["ema_decay"]: tf.train.ExponentialMovingAverage of the flat buffer, fp32 + its bf16 copy (6 bytes per parameter),
        # updated by one launch per optimizer step (DESIGN.md §4 "Weight EMA"); unset: no buffer, no launch
        self.ema = self.ema_b = None
        self._in_ema = False        # inside ema_weights(): pb / pbt hold the average
        self._ema_logged = False
        if self.ema_decay is not None:
            self._alloc_ema()
        self.global_step = 0
        # the masks of a training forward are keyed by (seed, global_step, microbatch, data-parallel rank, site); last_dropout =
        # {site: (key, thresh)} of the last one (empty with both rates 0).  _drop: the last forward was a dropped training forward.
        self.dropout_rank = int(self.hp.get("dp_rank") or 0)
        self.last_dropout: Dict[int, Tuple[int, int]] = {}
        self._microbatch = 0
        self._drop = False
        self._keep_pre = False      # qk_norm: the last forward was a training forward, which keeps the unnormalised q | k
        # state that comes into being on first use (None until then)
        self._t_table = None                      # refresh_compute_copies: the batched transpose's descriptor table
        self._kv = self._dec = None               # the sampler's key/value caches (under recompute_grad) and decode buffers
        # the engine's cache type -- what _prefill, the decode step and a sampling call without kv_cache_dtype use (kv_cache_as sets
        # it for a span) --, the FP8 caches (allocated on first use) and, inside an fp8 _prefill, the caches the forward quantises
        # every layer's k | v into
        self.kv_cache_dtype = KV_DEFAULT
        self._kv8 = self._kv8_out = None
        # token shift: the image grid's side, the sampler's history (hist[l][site], allocated on first use) and, inside _prefill,
        # the history the forward's shift launches also write
        self.G = grid_side(image_seq_len) if self.token_shift else None
        self._shift_hist = self._shift_hist_out = None
        self.gacc = self.loss_acc = self.loss_parts_acc = self.text_kept_frac_acc = None   # train_step's micro-batch accumulators
        self.event_hook = None                    # bench.py: a callable returning the list that takes the head launch's event pair
        self._ln_pend = []                        # LayerNorm gain / bias partials awaiting _flush_ln()
        self._build_attn_plans(attn_masks)
        # rotary embeddings: the (cos, sin) of every (position, pair), fp32 [S, head_dim / 2, 2], computed in float64 and uploaded once;
        # q | k of every projection buffer are rotated in place by dmi_rope_qk behind the QKV product, dqkv is rotated back behind
        # the attention backward (DESIGN.md §4 "Rotary"); off: no table, no launch
        self.rope_cs = None
        if self.rotary is not None:
            self.rope_cs = torch.from_numpy(rotary_table(self.rotary, self.T, self.S - self.T, self.hd, self.rotary_base)).to(self.dev)
        self._resolve_schedule()
        self._alloc_activations()
        # gradient exchange: RCCL behind the C ABI when `comm` (dp.init_comm) is given, torch.distributed otherwise
        self.reducer = GradReducer(self.g, world_size, comm=comm, pg=process_group)

    # ------------------------------------------------------------------ attention masks
    def _build_attn_plans(self, attn_masks):
        """attn_masks: None (every layer causal) or one bool [S, S] mask per layer (dalle_mtf.masks).  One device plan
        (dmi_attn_mask_plan) per distinct mask; causal layers keep plan None and call the causal entry points unchanged."""
        self.attn_plan = [None] * self.L
        if attn_masks is None:
            return
        if len(attn_masks) != self.L:
            raise ValueError(f"attn_masks: expected {self.L} per-layer masks, got {len(attn_masks)}")
        plans = {}
        for l, m in enumerate(attn_masks):
            m = np.ascontiguousarray(np.asarray(m, dtype=bool))
            key = (m.shape, hashlib.sha1(np.packbits(m)).hexdigest())
            if key not in plans:
                plans[key] = dh.AttnMaskPlan(m, device=self.dev)
            plan = plans[key]
            if plan.causal:
                continue
            if self.hd != 128:
                raise dh.DalleHipError(f"custom attention masks need head dim 128 (n_embd/n_heads = {self.hd}); "
                                       "the head-dim-64 kernels implement the causal mask only")
            self.attn_plan[l] = plan

    # layer l's attention: the causal entry, or the masked one with the layer's plan
    def _attn_fwd(self, l, qkv, o, lse):
        if self.attn_plan[l] is None:
            dh.attention_fwd(qkv, o, lse, self.B, self.H, self.S, head_dim=self.hd)
        else:
            dh.attention_fwd_masked(qkv, o, lse, self.attn_plan[l], self.B, self.H, self.S, head_dim=self.hd)

    def _attn_bwd(self, l):
        """self.dqkv from self.d_o and the block's stored q | k | v, output and log-sum-exp"""
        args = (self.qkv[l], self.o[l], self.d_o, self.lse[l], self.delta, self.dqkv)
        if self.attn_plan[l] is None:
            dh.attention_bwd(*args, self.B, self.H, self.S, head_dim=self.hd)
        else:
            dh.attention_bwd_masked(*args, self.attn_plan[l], self.B, self.H, self.S, head_dim=self.hd)

    def _attn_decode(self, l, cache, o, fresh, pos_dev):
        """one query row per sequence at the position in pos_dev against cache rows 0 .. pos; `fresh` (q | k | v of the step)
        enters the cache first.  Masked: the mask row of pos comes from the plan.  cache: the layer's bf16 [B*S, 3d] buffer, or the
        (data, scale) pair of its FP8 cache -- the one place that picks the decode entry point."""
        if isinstance(cache, tuple):
            dh.attention_decode_kv8(*cache, fresh, o, self.B, self.H, self.S, 0, pos_dev=pos_dev, head_dim=self.hd,
                                    plan=self.attn_plan[l])
        elif self.attn_plan[l] is None:
            dh.attention_decode(cache, o, self.B, self.H, self.S, 0, fresh=fresh, pos_dev=pos_dev, head_dim=self.hd)
        else:
            dh.attention_decode_masked(cache, o, self.attn_plan[l], self.B, self.H, self.S, 0, fresh=fresh, pos_dev=pos_dev,
                                       head_dim=self.hd)

    # ------------------------------------------------------------------ optimizer state
    OPTIMIZERS = ("adam", "adafactor")

    def set_optimizer(self, name):
        """allocates the state of the optimizer src/optimizers.py:78-99 selects ("optimizer", case-insensitive): Adam keeps m and v
        over the whole flat buffer; Adafactor keeps m (only when beta_1 != 0), a row and a column vector per factored variable and
        a full v only for the variables that do not factor (DESIGN.md §4 "Adafactor").  Re-selecting the current optimizer
        keeps its state; switching starts from zero state."""
        name = (name or "adam").lower()
        if name not in self.OPTIMIZERS:
            raise ValueError(f"{name} not recognized")
        if self.optimizer == name:
            return
        self.optimizer = name
        n = self.lay.total
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.m = self.v = self.af_slots = None
        if name == "adam":
            self.m = torch.zeros(n, **f32)
            self.v = torch.zeros(n, **f32)
            return
        table, self.af_vars, so = adafactor_table(self.lay)
        self.af_totals = dh.adafactor_plan(table)
        self.af_table = table.to(self.dev)
        self.af_ws = torch.empty(self.af_totals[2], dtype=torch.uint8, device=self.dev)
        self.af_slots = torch.zeros(max(so, 4), **f32)
        if self._af_beta1() != 0.0:
            self.m = torch.zeros(n, **f32)

    def _af_beta1(self):
        b1 = self.hp.get("beta_1")
        return 0.9 if b1 is None else float(b1)

    def export_adafactor_slots(self) -> "OrderedDict[str, np.ndarray]":
        """the Adafactor slots under mtf's names ([MTF-RECALL]): <var>_slot_vr (indexed along d1), <var>_slot_vc (along d0) for a
        factored variable, <var>_slot_v otherwise, and <var>_slot_m when beta_1 != 0"""
        assert self.optimizer == "adafactor"
        sl = self.af_slots.detach().cpu().numpy()
        mm = self.export_reference(self.m) if self.m is not None else None
        out: "OrderedDict[str, np.ndarray]" = OrderedDict()
        for r in self.af_vars:
            shp = r["shape"]
            if r["factored"]:
                R, C = shp
                vrow, vcol = sl[r["row"]:r["row"] + R].copy(), sl[r["col"]:r["col"] + C].copy()
                out[r["name"] + "_slot_vr"], out[r["name"] + "_slot_vc"] = (vrow, vcol) if r["vr_row"] else (vcol, vrow)
            else:
                out[r["name"] + "_slot_v"] = sl[r["v"]:r["v"] + int(np.prod(shp))].reshape(shp).copy()
            if mm is not None:
                out[r["name"] + "_slot_m"] = mm[r["name"]]
        return out

    def optimizer_buffers(self):
        """every device buffer of the optimizer state (the data-parallel start broadcasts them from rank 0)"""
        return [b for b in (self.m, self.v, self.af_slots) if b is not None]

    # ------------------------------------------------------------------ parameter access
    def view(self, buf, name):
        o = self.lay.offset[name]
        return buf[o:o + self.lay.numel(name)].view(self.lay.shape[name])

    def tview(self, name):
        o = self.lay.t_offset[name]
        r, c = self.lay.shape[name]
        return self.pbt[o:o + r * c].view(c, r)

    def _ref_view(self, buf, shp, off, ld):
        """a reference variable (a row of ParamLayout.reference_variables) as a strided view of a flat buffer"""
        return buf[off:].as_strided(shp, (ld, 1)[-len(shp):])

    def load_reference_params(self, P: Dict[str, np.ndarray]):
        """Load weights given under the reference's variable names/shapes."""
        with torch.no_grad():
            self.view(self.p, "to_logits/linear_out/kernel").zero_()
            self.view(self.p, "to_logits/linear_out/bias").fill_(-30000.0)   # pad logits can never win the softmax (and are masked in the CE kernel)
            for name, shp, off, ld in self.lay.reference_variables():
                if tuple(np.shape(P[name])) != tuple(shp) and "mlp_linear_1" in name:
                    raise ValueError(f"{name}: expected shape {tuple(shp)} with ff_glu {'on' if self.ff_glu else 'off'} "
                                     f"(got {tuple(np.shape(P[name]))}): the gated FFN's first layer is 8 n_embd wide, the plain one's 4")
                self._ref_view(self.p, shp, off, ld).copy_(torch.from_numpy(np.ascontiguousarray(P[name])).view(shp))
        self.refresh_compute_copies(cast=True)
        self._ema_from_p()

    def export_reference(self, buf=None) -> "OrderedDict[str, np.ndarray]":
        """Inverse of load_reference_params for any flat buffer (params, grads, m, v)."""
        buf = self.p if buf is None else buf
        return OrderedDict((name, np.ascontiguousarray(self._ref_view(buf, shp, off, ld).detach().float().cpu().numpy()))
                           for name, shp, off, ld in self.lay.reference_variables())

    # ------------------------------------------------------------------ weight EMA
    def _alloc_ema(self):
        self.ema = torch.zeros(self.lay.total, dtype=torch.float32, device=self.dev)
        self.ema_b = torch.zeros(self.lay.total, dtype=torch.bfloat16, device=self.dev)

    def _ema_from_p(self):
        """the average restarts from the parameters wherever they are set as a whole (pb = bf16(p) at that point)"""
        if self.ema is not None:
            self.ema.copy_(self.p)
            self.ema_b.copy_(self.pb)

    def _ema_update(self):
        """ema <- ema - (ema - p) * (1 - decay_t), t = the 0-based step of this update; behind the optimizer's launch.  An
        average that came with a checkpoint into a run without the key stays as loaded."""
        if self.ema_decay is not None:
            dh.ema_step(self.ema, self.p, self.ema_b, self.lay.total, one_minus_decay(self.ema_decay, self.global_step))

    @contextlib.contextmanager
    def ema_weights(self):
        """forward / evaluation / decode_step / sample_image_tokens inside the block compute from the averaged weights.  The
        average is COPIED into the storage of pb (and pbt re-derived from it by the batched transpose); the raw pb is stashed
        and copied back on exit.  No tensor is rebound: the captured decode graphs hold the addresses of pb and pbt.  p and
        the optimizer state are not touched; training inside the block raises RuntimeError."""
        if self.ema is None:
            raise ValueError("ema_weights(): this engine keeps no weight average (hparams['ema_decay'] is unset and no checkpoint "
                             "brought one)")
        if self._in_ema:            # nested: already computing from the average
            yield self
            return
        stash = self.pb.clone()
        self.pb.copy_(self.ema_b)
        self.refresh_compute_copies(cast=False)
        self._in_ema = True
        try:
            yield self
        finally:
            self.pb.copy_(stash)
            self.refresh_compute_copies(cast=False)
            self._in_ema = False

    def _not_in_ema(self, what):
        if self._in_ema:
            raise RuntimeError(f"{what} inside ema_weights(): the compute copies hold the averaged weights, not the ones being trained")

    def init_params(self, seed=1234):
        """Reference initialisers drawn with torch's generator on the host."""
        self.load_reference_params(reference_init(self.lay, self.H, seed))

    def refresh_compute_copies(self, cast=False):
        """bf16 natural copy (if not already written by the Adam kernel) + [out,in] copies for the fwd GEMMs."""
        if cast:
            dh.cast_f32_bf16(self.p, self.pb, self.lay.total)
        if self._t_table is None:   # one launch for all [in,out] -> [out,in] weight copies
            rows, tile = [], 0
            for name in self.lay.t_offset:
                r, c = self.lay.shape[name]
                rows.append([self.lay.offset[name], self.lay.t_offset[name], r, c, tile])
                tile += ((r + 63) // 64) * ((c + 63) // 64)
            self._t_table = torch.tensor(rows, dtype=torch.int64, device=self.dev)
            self._t_tiles = tile
        dh.transpose_batch(self.pb, self.pbt, self._t_table, self._t_table.shape[0], self._t_tiles)

    # ------------------------------------------------------------------ schedule switches
    def _resolve_schedule(self):
        """every choice between launch forms that holds for the engine's lifetime, resolved once before any buffer exists: an
        hparam wins, its environment variable gives the default, and a form also needs the library's own predicate for the
        shape.  DESIGN.md §4 "Engine schedule" has the table and the measurements behind the defaults."""
        hp, M, d = self.hp, self.M, self.d

        def switch(key, env):      # on unless the hparam, or failing that the environment variable ("0"), says off
            return bool(hp.get(key, os.environ.get(env, "1") != "0"))
        # recompute_grad (the reference wraps every block in mtf.recompute_grad, src/dalle_mtf/models.py:342-343): only the
        # residual stream X[l] is kept per layer; the block's inner activations live in ONE shared set of buffers and backward()
        # re-runs the block's forward (bit-identical kernels) before differentiating it
        self.recompute = bool(hp.get("recompute_grad", False))
        # dp_reserve_cus: CUs the persistent kernels of the BACKWARD leave to the RCCL channels of a concurrent gradient
        # exchange; data parallel only, 0 = off (the default: unmeasured on a multi-GPU node)
        self.dp_reserve_cus = int(hp.get("dp_reserve_cus", os.environ.get("DALLE_DP_RESERVE_CUS", "0"))) if self.world > 1 else 0
        # the FFN-1 product and the FFN-2 input gradient that matches it (_ffn1 / _ffn2_dgrad): GELU keeps the pre-activation
        # (it cannot be inverted from h); ReLU hands its mask on as one bit per element where the library runs both products on
        # the kernel that has the bit forms, and reads h back elsewhere (bit-identical).  ff_glu: FFN-1 is the plain product with its
        # bias at N = 8d into the stored pre = [value | gate]; dmi_glu_fwd / dmi_glu_bwd stand between it and FFN-2, no bit mask
        self.ffn_form = ("glu" if self.ff_glu else "gelu" if self.activation == "gelu" else
                         "relu_bits" if dh.relu_bits_auto(M, 4 * d, d) else "relu")
        self.use_relu_bits = self.ffn_form == "relu_bits"
        # the fused LayerNorm forms need the library's full-row kernel (n_embd = 512, operands inside its 32-bit offsets) and
        # no CUs reserved; the two-kernel forms serve every other case
        # (each asked with its widest product: forward FFN-2, K = 4d; backward FFN-1's input gradient, K = 4d or gated 8d)
        ln_ok = dh.gemm_nt_ln_auto(M, d, 4 * d) and self.dp_reserve_cus == 0
        lnbwd_ok = ln_ok and dh.gemm_nt_ln_auto(M, d, self.F1)
        # fuse_ln: the products that end in the residual stream emit the LayerNorm that follows them (dmi_gemm_nt_ln)
        self.fuse_ln = switch("fuse_ln", "DALLE_FUSE_LN") and ln_ok
        # FFN-2 -> next norm_1: not under recompute_grad, whose re-run of a block starts from the stored residual stream with a
        # standalone norm_1 (its statistics sum in another order; the re-run must reproduce the forward bit for bit)
        self.fuse_ln1 = self.fuse_ln and not self.recompute
        # fuse_lnbwd: LayerNorm backward inside the input-gradient product that feeds it (dmi_gemm_nt_lnbwd); dxn is never written
        # (not with token_shift: the shift's transpose stands between the product and the LayerNorm backward, and the fused form
        # cannot carry it -- the product lands in dxn, dmi_token_shift(inverse) and dmi_layernorm_bwd follow; with fuse_lnbwd go
        # the d_o chaining and the batched finish)
        self.fuse_lnbwd = switch("fuse_lnbwd", "DALLE_FUSE_LNBWD") and lnbwd_ok and not self.token_shift
        # lnbwd_batch_finish: the fused forms leave their gain / bias partials in one buffer per LayerNorm and ONE batched launch
        # sums them at the end of the backward (per block under data parallelism, where the exchange takes a block's gradients
        # as soon as it is done)
        self.lnb_batch = self.fuse_lnbwd and switch("lnbwd_batch_finish", "DALLE_LNBWD_BATCH")
        # dgrad_tail_split: the rows of the head input gradient's ragged last residency run with K split (_backward)
        self.dgrad_tail_split = switch("dgrad_tail_split", "DALLE_DGRAD_TAIL")
        # decode_fuse_ln: the decode step's LayerNorms ride in the prologue of the product that reads them (_decode_body)
        self.decode_fuse_ln = bool(hp.get("decode_fuse_ln", True))
        # all FOUR weight gradients of a block in one launch where the library's plan for the four is the wide (128 x 256)
        # tile; elsewhere (n_embd = 1024 / 2048: 384+ tiles, ragged residencies in ONE launch) the attention pair shares a
        # launch and the FFN gradients keep their own
        # (wgrad_shapes: (I, J) of the four in the order of _wgrad_problems and ws_blk -- FFN-2, FFN-1, out-projection, QKV)
        self.wgrad_shapes = [(4 * d, d), (d, self.F1), (d, d), (d, 3 * d)]
        self.wgrad_group4 = dh.gemm_tn_group_plan(self.wgrad_shapes, M) > 0

    # ------------------------------------------------------------------ buffers
    def _alloc_activations(self):
        M, d, L, B, H, S, Vp = self.M, self.d, self.L, self.B, self.H, self.S, self.Vp
        b16 = dict(dtype=torch.bfloat16, device=self.dev)
        f32 = dict(dtype=torch.float32, device=self.dev)
        u8 = dict(dtype=torch.uint8, device=self.dev)
        self.tokens = torch.zeros(B, S, dtype=torch.int32, device=self.dev)
        self.labels = torch.zeros(B, S, dtype=torch.int32, device=self.dev)
        self.X = [torch.empty(M, d, **b16) for _ in range(L + 1)]       # residual stream entering layer l
        nl = 1 if self.recompute else L     # recompute_grad: 0.63 GB -> 0.1 GB per layer at B=32, S=1280

        def per_layer(make):
            bufs = [make() for _ in range(nl)]
            return [bufs[l % nl] for l in range(L)]
        self.xn1 = per_layer(lambda: torch.empty(M, d, **b16))
        self.qkv = per_layer(lambda: torch.empty(M, 3 * d, **b16))
        # qk_norm: the unnormalised q | k of every row, what dmi_qk_norm_bwd recomputes the statistics from (L * M * 2d * 2 bytes, one
        # shared buffer under recompute_grad; DESIGN.md §4 "QK norm"); off: nothing
        self.qk_pre = per_layer(lambda: torch.empty(M, 2 * d, **b16)) if self.qk_norm else None
        self.o = per_layer(lambda: torch.empty(M, d, **b16))
        self.lse = per_layer(lambda: torch.empty(B, H, S, **f32))
        self.x1 = per_layer(lambda: torch.empty(M, d, **b16))
        self.xn2 = per_layer(lambda: torch.empty(M, d, **b16))
        self.h = per_layer(lambda: torch.empty(M, 4 * d, **b16))
        # what FFN-1 keeps beside h for the FFN-2 input gradient: the ReLU mask as bits (M * 4d / 8 bytes instead of a read of h,
        # 168 MB per layer at dalle_example) or GELU's pre-activation a = xn2 . W1 + b1 (bf16, 2 bytes per hidden element)
        self.hbits = per_layer(lambda: torch.empty(dh.relu_bits_bytes(M, 4 * d), **u8)) if self.ffn_form == "relu_bits" else None
        # or the gated FFN's [value | gate] (8d wide)
        self.hpre = (per_layer(lambda: torch.empty(M, self.F1 if self.ffn_form == "glu" else 4 * d, **b16))
                     if self.ffn_form in ("gelu", "glu") else None)
        self.stats = per_layer(lambda: [torch.empty(M, **f32) for _ in range(4)])  # mean1, rstd1, mean2, rstd2
        self.xnf = torch.empty(M, d, **b16)
        # token shift: xn1[l] / xn2[l] hold the SHIFTED rows -- what the QKV product, FFN-1 and their weight gradients read.  The
        # LayerNorm that produces them (standalone, fused into a product, or dmi_dropout_add_ln) writes into this one scratch buffer
        # and dmi_token_shift follows; the backward brings dxn back through it (_ln_dgrad).  xnf is not shifted.
        self.shift_tmp = torch.empty(M, d, **b16) if self.token_shift else None
        self.statf = [torch.empty(M, **f32) for _ in range(2)]
        self.z = torch.empty(M, Vp, **b16)      # eval: logits; train: E = exp(logit), patched into unnormalised dlogits
        self.loss_rows = torch.empty(M, **f32)
        self.loss = torch.zeros(1, **f32)
        # hparams["text_loss_weight"] / ["image_loss_weight"] (dalle_mtf.loss_weights): the static weight of every position, computed
        # in float64 and uploaded once; loss3 = (weighted loss | text mean, image mean), written by dmi_loss_reduce
        self.pos_weight = self.loss_parts = None
        if self.loss_weights is not None and not self.loss_ignore_padding:
            w = position_weights(self.T, S - self.T, *self.loss_weights)
            self.pos_weight = torch.from_numpy(w.astype(np.float32)).to(self.dev)
            self.loss3 = torch.zeros(3, **f32)
            self.loss, self.loss_parts = self.loss3[0:1], self.loss3[1:3]
        # hparams["loss_ignore_padding"] (dalle_mtf.loss_mask): the weight of a row depends on its label, so dmi_loss_mask writes
        # row_w [M] and counts = (kept text rows, image rows) behind shift_labels in every forward, the weighted finish reads row_w
        # with period M, and dmi_loss_reduce_masked writes loss4 = (loss | kept-text mean, image mean | kept fraction of the text
        # labels).  The counts stay on the device.  Off: none of these buffers, none of these launches
        self.row_w = self.mask_counts = self.text_kept_frac = None
        if self.loss_ignore_padding:
            self.mask_coef = mask_coefficients(self.loss_weights)
            self.row_w = torch.zeros(M, **f32)
            self.mask_counts = torch.zeros(2, dtype=torch.int32, device=self.dev)
            self.loss4 = torch.zeros(4, **f32)
            self.loss, self.loss_parts, self.text_kept_frac = self.loss4[0:1], self.loss4[1:3], self.loss4[3:4]
        self.gnorm_sq = torch.zeros(1, **f32)
        # fused softmax head (training path, include/dalle_hip.h K7/K8 (b))
        self.nparts = dh.gemm_nt_softmax_partials(Vp)
        self.zl = torch.empty(M, **f32)                      # label logit (loss = logsumexp - label logit)
        self.rowsum_part = torch.empty(self.nparts, M, **f32)
        self.rowscale = torch.empty(M, **f32)                # dz_scale / sum_v exp(.)
        self.rowscale_bf = torch.empty(_round_up(M, 128) + 128, **b16)
        self.xs = torch.empty(M, d, **b16)                   # rowscale * LN_f(x): left operand of the head weight gradient
        self.head_flag = torch.zeros(1, dtype=torch.int32, device=self.dev)
        # token-id order for the embedding scatter-add: sorted on a side stream while the forward runs
        self.tok_sorted = torch.empty(M, dtype=torch.int32, device=self.dev)
        self.tok_perm = torch.empty(M, dtype=torch.int32, device=self.dev)
        self.sort_ws = torch.empty(dh.sort_tokens_workspace_bytes(M), **u8)
        self.embed_ws = torch.empty(dh.embed_bwd_workspace_bytes(B, S, d), **u8)
        self.sort_stream = torch.cuda.Stream(device=self.dev)
        self._sort_done = None
        # scratch
        self.dx = [torch.empty(M, d, **b16) for _ in range(2)]
        self.dxn = torch.empty(M, d, **b16)
        self.dh = torch.empty(M, 4 * d, **b16)
        # gated FFN: the gradient of pre = [value | gate], what FFN-1's input, weight and bias gradients read in place of dh
        self.dpre = torch.empty(M, self.F1, **b16) if self.ffn_form == "glu" else None
        self.dqkv = torch.empty(M, 3 * d, **b16)
        self.d_o = torch.empty(M, d, **b16)
        # residual dropout: drop_y is where the out-projection and FFN-2 land (bias only) before dmi_dropout_add_ln, in the forward
        # and in its re-run; dyd are the masked gradients of the two branch outputs (dya -> FFN-2, dyb -> out-projection), which
        # must stay untouched until the block's grouped weight-gradient launch behind the attention backward
        self.drop_y = torch.empty(M, d, **b16) if self.resid_thresh else None
        self.dyd = [torch.empty(M, d, **b16) for _ in range(2)] if self.resid_thresh else None
        self.delta = torch.empty(3, B, H, S, **f32)   # delta | (lse, delta) pairs for the dK/dV kernel's DMA
        wsz = max(dh.gemm_tn_workspace_bytes(M, d, Vp), *(dh.gemm_tn_workspace_bytes(M, i_, j_) for i_, j_ in self.wgrad_shapes),
                  dh.layernorm_bwd_workspace_bytes(M, d), dh.sumsq_workspace_bytes(self.lay.total),
                  dh.gemm_nt_splitk_workspace_bytes(M // 2 + 256, d, 8),
                  dh.qk_norm_bwd_workspace_bytes(M, self.hd) if self.qk_norm else 0)
        self.ws = torch.empty(int(wsz) + 1024, **u8)
        # the four weight gradients of a block keep their split-m slabs in separate workspaces and their seven slab reduces
        # run as ONE launch at the end of the block's backward (dmi_reduce_slabs_batch)
        self.ws_blk = [torch.empty(int(dh.gemm_tn_workspace_bytes(M, i_, j_)) + 256, **u8) for i_, j_ in self.wgrad_shapes]
        self.deferred = dh.DeferredReduces()
        if self.fuse_lnbwd:
            npart = dh.gemm_nt_lnbwd_parts(M) * 2 * d
            self.lnb_part = [torch.empty(npart, **f32) for _ in range(2 * L if self.lnb_batch else 1)]
            self.ln_ws_final = torch.empty(int(dh.layernorm_bwd_workspace_bytes(M, d)) + 256, **u8)

    # ------------------------------------------------------------------ forward
    def _w(self, name):
        return self.view(self.pb, name)

    def forward(self, tokens: torch.Tensor, need_grad=True) -> torch.Tensor:
        """tokens int32 [B,S] on device.  Returns the device scalar loss = mean over ALL B*S positions of
        -log softmax(logits)[label] (src/dalle_mtf/models.py:348-359), labels = shift(tokens) (:407-410).
        With loss weights set (self.pos_weight): the weighted loss sum_{b,p} w[p] NLL[b,p] / B instead, self.loss_parts = the
        unweighted (text mean, image mean), and rowscale carries w[p]; self.loss_rows stays the unweighted NLL.
        With "loss_ignore_padding" on (self.row_w): the masked loss sum_{b,p} c[b,p] NLL[b,p] of dalle_mtf.loss_mask, with or without
        loss weights; self.loss_parts = (mean over the kept caption labels, image mean), self.text_kept_frac the kept fraction of the
        caption labels, rowscale carries c[b,p] (0 on ignored rows); self.loss_rows stays the unmasked NLL of every position.
        need_grad=True (training): the softmax is fused into the vocabulary projection -- self.z then holds the
        unnormalised dlogits E, self.rowscale their per-row factor (already scaled by 1/(global B*S*microbatches)).
        need_grad=False (evaluation): self.z holds the bf16 logits (see logits()); the loss is the plain mean
        (the reference forces num_microbatches = 1 outside training, src/model_fns.py:150-154)."""
        B, S, L = self.B, self.S, self.L
        assert tokens.shape == (B, S) and tokens.dtype == torch.int32
        self.tokens.copy_(tokens)
        self._keep_pre = bool(need_grad)
        self._sort_done = None
        if need_grad:   # token-id order for the embedding backward: twelve 3-5 us launches on a side stream (see dmi_sort_tokens)
            self._launch_sort()
        dh.shift_labels(self.tokens, self.labels, B, S, self.eos)
        if self.row_w is not None:   # this batch's row weights and counts (text rows: p < T - 1)
            ct, ci, plain = self.mask_coef
            dh.loss_mask(self.labels, self.M, S, self.T - 1, self.loss_pad_id, ct, ci, plain, self.mask_counts, self.row_w)
        self._draw_dropout(need_grad)
        self._embed_fwd()
        for l in range(L):
            self._block_forward(l)
        self._ln_of_stream(L)
        return self._loss_head(need_grad)

    def _loss_head(self, need_grad):
        """xnf -> the loss (and, training, what the head's backward reads: see forward)"""
        M, d, S, Vp = self.M, self.d, self.S, self.Vp
        Wt, bias = self.tview("to_logits/linear_out/kernel"), self._w("to_logits/linear_out/bias")
        nmb = (self.hp.get("num_microbatches", 1) or 1) if need_grad else 1
        weighted, masked = self.pos_weight is not None, self.row_w is not None
        if need_grad:
            dh.label_logit(self.xnf, d, Wt, d, bias, self.labels, self.zl, self.head_flag, M, d, self.V)
        hook = self.event_hook       # bench.py: HIP events around the largest single launch
        if hook is not None:
            e0 = torch.cuda.Event(enable_timing=True)
            e0.record()
        if need_grad:
            dh.gemm_nt_softmax(self.xnf, d, Wt, d, bias, None, self.z, Vp, self.rowsum_part, M, Vp, d)   # no exponent shift
        else:
            dh.gemm_nt(self.xnf, d, Wt, d, self.z, Vp, M, Vp, d, dh.GEMM_BIAS, bias=bias)
        if hook is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record()
            hook().append((e0, e1))
        if need_grad:   # the weighted finish scales row (b, p) by w[p] / (global B), the plain one every row by 1 / (global B * S)
            if masked:  # row_w is normalised by this forward's own counts: what is left is the mean over micro-batches and ranks
                finish, scale = dh.softmax_finish_w, (1.0 / (nmb * self.world), self.row_w, M)
            else:
                finish, scale = ((dh.softmax_finish_w, (1.0 / (self.B_global * nmb), self.pos_weight, S)) if weighted else
                                 (dh.softmax_finish, (1.0 / (self.B_global * S * nmb),)))
            finish(self.rowsum_part, self.nparts, self.zl, None, self.labels, self.xnf, d, Wt, d, bias, self.z, Vp, Vp,
                   self.loss_rows, self.rowscale, self.rowscale_bf, self.xs, self.head_flag, M, d, self.V, *scale)
        else:
            dh.cross_entropy(self.z, Vp, self.labels, self.loss_rows, None, M, self.V, 0.0)
        if masked:
            dh.loss_reduce_masked(self.loss_rows, self.row_w, self.labels, M, S, self.T - 1, self.loss_pad_id, self.mask_counts,
                                  1.0 / nmb, self.loss4)
        elif weighted:
            dh.loss_reduce(self.loss_rows, M, self.pos_weight, S, self.T - 1, 1.0 / (self.B * nmb), self.loss3)
        else:
            dh.sum_f32(self.loss_rows, M, 1.0 / (M * nmb), self.loss)
        return self.loss

    def _draw_dropout(self, training):
        """the keys of this forward's masks: a training forward with a rate above 0 draws one per site, anything else none"""
        self._drop = bool(training and (self.embed_thresh or self.resid_thresh))
        self.last_dropout = {}
        if not self._drop:
            return
        key = lambda site: site_key(self.dropout_seed, self.global_step, self._microbatch, self.dropout_rank, site)   # noqa: E731
        if self.embed_thresh:
            self.last_dropout.update({s_: (key(s_), self.embed_thresh) for s_ in (SITE_TOKEN, SITE_POSITION)})
        if self.resid_thresh:
            for l in range(self.L):
                self.last_dropout.update({s_: (key(s_), self.resid_thresh) for s_ in (site_attention(l), site_mlp(l))})

    def _drop_resid(self):
        return self._drop and self.resid_thresh > 0

    def _embed_args(self):
        """the trailing arguments of the embedding's dropout entries: (token key, position key, threshold), or () undropped"""
        if not (self._drop and self.embed_thresh):
            return ()
        return self.last_dropout[SITE_TOKEN][0], self.last_dropout[SITE_POSITION][0], self.embed_thresh

    def _embed_fwd(self):
        drop = self._embed_args()
        (dh.embed_fwd_dropout if drop else dh.embed_fwd)(self.tokens, self._w("embedding/wte"), self._w("positional_embedding/wpe"),
                                                         self.X[0], self.S, self.d, self.V, *drop)

    def _embed_bwd(self, dx):
        drop = self._embed_args()
        (dh.embed_bwd_dropout if drop else dh.embed_bwd)(self.tok_sorted, self.tok_perm, dx, self._gv("embedding/wte"),
                                                         self._gv("positional_embedding/wpe"), self.B, self.S, self.d, self.V,
                                                         self.embed_ws, *drop)

    # ---- the LayerNorm that reads the stream leaving a block
    def _ln_after(self, l):
        """(gain, bias, y, mean, rstd) of the LayerNorm that reads X[l + 1]: norm_1 of block l + 1, to_logits' after the last"""
        if l + 1 < self.L:
            q, y, (mean, rstd) = f"layer_{l + 1}/norm_1/", self._ln_y(self.xn1[l + 1]), self.stats[l + 1][:2]
        else:
            q, y, (mean, rstd) = "to_logits/layer_norm/", self.xnf, self.statf
        return self._w(q + "g"), self._w(q + "b"), y, mean, rstd

    def _ln_y(self, xn):
        """where a block LayerNorm writes its output for xn (an xn1[l] / xn2[l]): xn itself, or with token_shift the scratch
        buffer that _shift_ln then shifts into xn"""
        return self.shift_tmp if self.token_shift else xn

    def _shift_ln(self, l, site):
        """token_shift: xn1[l] (site 0) / xn2[l] (site 1) = shift of the LayerNorm output in the scratch buffer; inside _prefill
        the launch also writes the sampler's history of (l, site).  Off: nothing."""
        if self.token_shift:
            hist = self._shift_hist_out[l][site] if self._shift_hist_out is not None else None
            dh.token_shift(self.shift_tmp, (self.xn2 if site else self.xn1)[l], self.M, self.S, self.T, self.G, self.d, hist=hist)

    def _ln1_by_prev(self):
        """norm_1 of block l + 1 (and to_logits' norm) is written by block l's FFN-2: the fused product, or under residual dropout
        dmi_dropout_add_ln -- neither under recompute_grad, whose re-run starts from a standalone norm_1"""
        return self.fuse_ln1 or (self._drop_resid() and not self.recompute)

    def _ln_of_stream(self, l):
        """the LayerNorm that reads X[l] on its own launch -- unless block l - 1's FFN-2 has written it"""
        if not (self._ln1_by_prev() and l > 0):
            g, b, y, mean, rstd = self._ln_after(l - 1)
            dh.layernorm_fwd(self.X[l], g, b, y, mean, rstd, self.M, self.d)
            if l < self.L:
                self._shift_ln(l, 0)

    def _join_branch(self, l, mlp):
        """a branch of block l joins the residual stream, and the LayerNorm that reads the sum: the out-projection (x1 = X[l] + ..,
        read by norm_2) or, mlp, FFN-2 (X[l + 1] = x1 + .., read by _ln_after(l) where this launch is to write it: _ln1_by_prev).
        Residual dropout (a training forward, and its re-run): the product runs with its bias only into a scratch buffer and
        dmi_dropout_add_ln drops, adds and normalises in one pass at every width; the keys are last_dropout's, so the re-run
        restates the same masks.  fuse_ln: full-row tiles emit the LayerNorm in the product's pass (dmi_gemm_nt_ln)."""
        M, d, p, st = self.M, self.d, f"layer_{l}/", self.stats[l]
        if mlp:
            A, K, W, bias = self.h[l], 4 * d, self.tview(p + "mlp/mlp_linear_2/kernel"), self._w(p + "mlp/mlp_linear_2/bias")
            res, out, site = self.x1[l], self.X[l + 1], site_mlp(l)
            ln = self._ln_after(l) if self._ln1_by_prev() else None
        else:
            A, K, W, bias = self.o[l], d, self.tview(p + "attn/o"), self._w(p + "attn/compute_output_bias/o_b")
            res, out, site = self.X[l], self.x1[l], site_attention(l)
            ln = (self._w(p + "norm_2/g"), self._w(p + "norm_2/b"), self._ln_y(self.xn2[l]), st[2], st[3])
        if self._drop_resid():
            dh.gemm_nt(A, K, W, K, self.drop_y, d, M, d, K, dh.GEMM_BIAS, bias=bias)
            dh.dropout_add_ln(self.drop_y, res, out, *(ln or (None,) * 5), M, d, *self.last_dropout[site])
        elif self.fuse_ln and ln is not None:
            g, b, y, mean, rstd = ln
            dh.gemm_nt_ln(A, K, W, K, out, d, M, d, K, g, b, y, d, mean, rstd, bias=bias, residual=res)
        else:
            dh.gemm_nt(A, K, W, K, out, d, M, d, K, dh.GEMM_BIAS | dh.GEMM_RESIDUAL, bias=bias, residual=res)
            if ln is not None:
                g, b, y, mean, rstd = ln
                dh.layernorm_fwd(out, g, b, y, mean, rstd, M, d)
        if ln is not None and not mlp:
            self._shift_ln(l, 1)
        elif ln is not None and l + 1 < self.L:
            self._shift_ln(l + 1, 0)

    # ---- FFN-1 and the FFN-2 input gradient, one arm of self.ffn_form each
    def _ffn1(self, l):
        """h = act(xn2 . W1^T + b1), and what the form keeps for _ffn2_dgrad: the pre-activation, the mask bits, or nothing.
        glu: pre = xn2 . W1^T + b1 at width 8d (the plain product), then h = pre[:, :4d] * act(pre[:, 4d:])"""
        M, d, p = self.M, self.d, f"layer_{l}/"
        args = (self.xn2[l], d, self.tview(p + "mlp/mlp_linear_1/kernel"), d, self.h[l], 4 * d, M, 4 * d, d)
        b1 = self._w(p + "mlp/mlp_linear_1/bias")
        if self.ffn_form == "glu":
            dh.gemm_nt(*args[:4], self.hpre[l], self.F1, M, self.F1, d, dh.GEMM_BIAS, bias=b1)
            dh.glu_fwd(self.hpre[l], self.F1, self.h[l], 4 * d, M, 4 * d, self.activation)
        elif self.ffn_form == "gelu":
            dh.gemm_nt_gelu(*args, b1, self.hpre[l], 4 * d)
        elif self.ffn_form == "relu_bits":
            dh.gemm_nt_relu_bits(*args, b1, self.hbits[l])
        else:
            dh.gemm_nt(*args, dh.GEMM_BIAS | dh.GEMM_RELU, bias=b1)

    def _ffn2_dgrad(self, l, dy):
        """self.dh = (dy . W2^T) * act'(..): gelu' of the stored pre-activation, the mask bits, or h > 0 read back from h.
        glu: self.dh = dy . W2^T, the plain product, and self.dpre = its gradient w.r.t. [value | gate] (_ffn1_grad_in)"""
        M, d = self.M, self.d
        args = (dy, d, self._w(f"layer_{l}/mlp/mlp_linear_2/kernel"), d, self.dh, 4 * d, M, 4 * d, d)
        if self.ffn_form == "glu":
            dh.gemm_nt(*args)
            dh.glu_bwd(self.dh, 4 * d, self.hpre[l], self.F1, self.dpre, self.F1, M, 4 * d, self.activation)
        elif self.ffn_form == "gelu":
            dh.gemm_nt_gelu_grad(*args, self.hpre[l], 4 * d)
        elif self.ffn_form == "relu_bits":
            dh.gemm_nt_mask_bits(*args, self.hbits[l])
        else:
            dh.gemm_nt(*args, dh.GEMM_RELU_MASK, relu_src=self.h[l])

    def _ffn1_grad_in(self):
        """the gradient of FFN-1's output, [M, F1]: what its input, weight and bias gradients read"""
        return self.dpre if self.ffn_form == "glu" else self.dh

    def _block_forward(self, l, rerun=False):
        """one transformer block (src/dalle_mtf/models.py:326-335): X[l] -> X[l+1].  rerun: what backward() re-runs under
        recompute_grad -- the block's inner activations up to h; X[l+1] is already stored."""
        M, d, p = self.M, self.d, f"layer_{l}/"
        self._ln_of_stream(l)
        dh.gemm_nt(self.xn1[l], d, self.tview(p + "attn/qkv"), d, self.qkv[l], 3 * d, M, 3 * d, d)
        if self.qk_norm:               # normalised, and with rotary rotated in the same pass; a training forward keeps the input
            dh.qk_norm_fwd(self.qkv[l], *self._qk_gains(l), M, self.S, self.H, self.hd,
                           pre=self.qk_pre[l] if self._keep_pre or rerun else None, cs=self.rope_cs)
        elif self.rope_cs is not None:   # the attention kernels, their backward and the decode caches see rotated q and k
            dh.rope_qk(self.qkv[l], self.rope_cs, M, self.S, self.H, self.hd)
        if self._kv8_out is not None:    # an fp8 prefill: the layer's q | k | v are final, its k | v rows enter the FP8 cache
            dh.kv8_quantize(self.qkv[l], *self._kv8_out[l], self.B, self.S, self.H, self.hd, 0, self.S)
        self._attn_fwd(l, self.qkv[l], self.o[l], self.lse[l])   # no transposed copies: hardware transpose reads
        self._join_branch(l, mlp=False)
        self._ffn1(l)
        if not rerun:
            self._join_branch(l, mlp=True)

    def _qk_gains(self, l, buf=None):
        """qk_norm: layer l's (q gain, k gain), [head_dim] each, in the bf16 compute copy (or in flat buffer `buf`)"""
        return tuple(self.view(self.pb if buf is None else buf, f"layer_{l}/{g}") for g in GAIN_NAMES)

    def logits(self) -> torch.Tensor:
        """fp32 logits [B,S,V] of the last forward(need_grad=False) ("go to full precision", models.py:395)."""
        # (after a training forward self.z holds unnormalised dlogits, not logits)
        return self.z.view(self.B, self.S, self.Vp)[:, :, :self.V].float()

    # ------------------------------------------------------------------ sampling
    def sample_image_tokens(self, text: torch.Tensor, temperature: float = 1.0, top_k: int = 0, seed: int = 0,
                            top_p: float = 1.0, image_prefix: Optional[torch.Tensor] = None, return_logprobs: bool = False,
                            kv_cache: bool = True, decode_graph: bool = True, fused_sampling: bool = True,
                            guidance_scale: float = 1.0, uncond_text: Optional[torch.Tensor] = None, weights: Optional[str] = None,
                            kv_cache_dtype: Optional[str] = None):
        """Autoregressive image-token sampling: text int32 [B, T] -> image-token ids [B, P] in [0, image_vocab_size).
        The reference scaffolds this (is_incremental_inference, models.py:246-254,281-285) but its predict path raises
        NotImplementedError (model_fns.py:135-136).  Logits are restricted to the image vocabulary; temperature / top-k /
        greedy (temperature 0) / nucleus (top_p < 1).

        kv_cache=True (default): ONE full forward over the text prefix fills the per-layer key/value cache (the [B*S, 3d]
        projection buffers of the forward pass), then every further token is one incremental step over B rows --
        decode_step(): QKV GEMM writing row `pos` of the cache in place, dmi_attention_decode (one query against keys
        0..pos), out-projection, MLP -- ~90 launches of a few microseconds instead of a 1280-position forward, replayed as
        one HIP graph (decode_graph; see decode_step).
        Under recompute_grad the forward keeps ONE shared set of projection buffers, so the sampler allocates its own
        per-layer caches on the first cached call and keeps them for later calls: L * B * S * 3d * 2 bytes (dalle_coco at
        B = 128: 12 GB); the prefill forward writes into them.  Training buffers are not touched.
        fused_sampling (with kv_cache and decode_graph): the draw itself is a kernel at the end of the replayed graph
        (dmi_sample_tokens: temperature / top-k / Gumbel-max categorical draw, noise a pure function of (seed, position, row))
        that writes the chosen token where the next step's embedding reads it -- P graph replays back to back, no host round
        trip per position.  fused_sampling=False launches the same draw kernel from the host after each decode step (same
        tokens for the same seed: the noise is a pure function of (seed, position, row, index)).
        kv_cache=False: the plain form, one full evaluation forward per generated position (the causal mask makes the
        not-yet-generated tail irrelevant); kept as the cross-check the cached path is tested against.

        top_p < 1 or return_logprobs=True draw with dmi_sample_tokens_p (nucleus filter after top-k; same noise, so top_p = 1
        gives the same tokens); otherwise the launches are exactly those above.  return_logprobs=True returns (tokens,
        logp fp32 [B]): the sum over the drawn positions of log softmax(logits over the image vocabulary)[token] at
        temperature 1, unfiltered -- the model's own score of each sample.
        image_prefix (int [B, k], ids in [0, image_vocab_size), 0 <= k < P): image completion.  The returned tokens start with
        the prefix; positions T-1 .. T+k-2 go through the same decode steps as sampled positions, teacher-forced (the
        decode_step body), and drawing starts at position T+k-1 -- so sampling s and then completing s[:, :k] returns s
        bit for bit.  Prefix tokens are not drawn and add nothing to logp.

        Classifier-free guidance (guidance_scale != 1 or uncond_text given; with both at their defaults every launch is as
        above): the engine's B rows are Bc = B // 2 pairs.  text is [Bc, T] and fills rows 0 .. Bc-1; rows Bc .. B-1 take
        uncond_text (int [T] or [Bc, T]; default the null caption, T copies of hparams["padding_id"], or of
        text_vocab_size - 1 when that is unset -- the padding rule of src/input_fns.py, which is also what "caption_dropout"
        trains on).  The decode step is row-independent, so both halves ride through the same prefill and decode graph; the
        draw is dmi_sample_tokens_guided (include/dalle_hip.h) on every path: pair b draws ONE token from
        l_uncond + guidance_scale * (l_cond - l_uncond) and both rows are fed it.  image_prefix is [Bc, k] and is
        teacher-forced into both halves.  Returns tokens [Bc, P] (and logp [Bc]: the conditional rows' own log-likelihood of
        the drawn tokens, unguided, temperature 1).

        weights: "ema" samples from the weight average (inside ema_weights()), "raw" from the raw iterate, None from the
        average when the engine has one.  "ema" without an average raises ValueError.

        kv_cache_dtype: "bf16" or "fp8" (None: the engine's, self.kv_cache_dtype, "bf16" unless set).  "fp8": K and V of every
        layer in OCP E4M3 with one power-of-two scale per (position, head) (include/dalle_hip.h "kv8"; DESIGN.md §4 "Generation: FP8 key/value cache"): the prefill's forward
        quantises each layer's rows behind its QKV product (dmi_kv8_quantize), the decode step attends with
        dmi_attention_decode_kv8, and every key and value the attention sees is a dequantised one.  L * B * S * (2d + 8H) bytes,
        allocated once; under recompute_grad the bf16 caches above are never allocated.  Every other argument composes unchanged;
        logp is then the likelihood under the fp8-cache computation.  Anything else, or "fp8" with kv_cache=False: ValueError."""
        kv_dtype = resolve_kv_cache_dtype(self.kv_cache_dtype if kv_cache_dtype is None else kv_cache_dtype, kv_cache)
        which = resolve_weights(weights, self.ema is not None)
        if which == "raw" and self._in_ema:
            raise RuntimeError("sample_image_tokens(weights='raw') inside ema_weights(): the compute copies hold the average")
        a = check_sample_args(self.B, self.T, self.S - self.T, self.text_vocab_size, self.image_vocab_size, text, top_p=top_p,
                              guidance_scale=guidance_scale, uncond_text=uncond_text, image_prefix=image_prefix,
                              padding_id=self.hp.get("padding_id"))
        with self.ema_weights() if which == "ema" else contextlib.nullcontext(), self.kv_cache_as(kv_dtype):
            return self._sample(text, a, temperature, top_k, seed, return_logprobs, kv_cache, decode_graph, fused_sampling)

    def _sample(self, text, a, temperature, top_k, seed, return_logprobs, kv_cache, decode_graph, fused_sampling):
        """the body of sample_image_tokens on checked arguments (a: SampleArgs), from whichever weights pb / pbt hold"""
        B, T, S, P = self.B, self.T, self.S, self.S - self.T
        R, guided, gs, top_p, uncond_text, image_prefix, k = a
        lo, hi = self.text_vocab_size, self.text_vocab_size + self.image_vocab_size
        nv = hi - lo
        variant = Draw(nucleus=guided or top_p < 1.0 or return_logprobs, guided=guided, logp=return_logprobs)
        toks = torch.full((B, S), lo, dtype=torch.int32, device=self.dev)
        toks[:R, :T] = text.to(device=self.dev, dtype=torch.int32)
        if guided:
            toks[R:, :T] = uncond_text.to(device=self.dev, dtype=torch.int32)       # [T] broadcasts over the rows
        if k:
            toks[:R, T:T + k] = image_prefix.to(device=self.dev, dtype=torch.int32) + lo
            if guided:
                toks[R:, T:T + k] = toks[:R, T:T + k]
        logp = torch.zeros(R, dtype=torch.float32, device=self.dev) if return_logprobs else None

        def result(img):
            return (img, logp) if return_logprobs else img

        if kv_cache and decode_graph and fused_sampling and nv <= 8192:
            self._prefill(toks)                          # k, v of the text positions are in the cache
            D = self._decode_state()
            for pos in range(T - 1, T - 1 + k):          # the prefix, teacher-forced through the decode step
                self.decode_step(toks[:, pos].contiguous(), pos, graph=True)
            D["tok"].copy_(toks[:, T - 1 + k])
            D["pos_i"][0:1].fill_(T - 1 + k)
            prm = draw_params(variant, temperature, top_k, seed, top_p, gs)
            D["params"][:prm.numel()].copy_(prm)         # the plain draw has four words and leaves words 4, 5 alone
            if return_logprobs:
                D["logp"].zero_()
            for _ in range(P - k):                       # position T-1+i predicts image token i; the graph advances the position itself
                self._run_decode(sample=variant, graph=True)
            img = D["out"][:R].clone()                   # guided: the kernel writes one row per pair
            if k:
                img[:, :k] = toks[:R, T:T + k] - lo
            if return_logprobs:
                logp.copy_(D["logp"][:R])
            return result(img)

        if nv > 8192:
            raise dh.DalleHipError(f"sample_image_tokens: the draw kernel (dmi_sample_tokens) handles image vocabularies up to 8192 (got {nv})")
        bias = self._w("to_logits/linear_out/bias")[lo:hi]
        nxt = torch.empty(B, dtype=torch.int32, device=self.dev)

        def pick(z, ldz, zbias, position):
            """the draw itself is the same kernel on every path (temperature / top-k / Gumbel-max with counter-based noise
            hash(seed, position, row, index), first maximum when temperature <= 0): host-launched here, the last node of the
            replayed graph on the fused path -- the same (seed, position) gives the same draw on both."""
            self._draw(variant, z, ldz, zbias, nxt, logp, top_p=top_p, scale=gs, temperature=temperature, top_k=top_k, seed=seed,
                       pos=position)
            return nxt

        for pos in range(P):
            if not kv_cache:
                if pos < k:
                    continue                             # the causal mask: a full forward needs no steps over the prefix
                self.forward(toks, need_grad=False)
                # the position before predicts token T + pos; the evaluation head already carries the bias (GEMM epilogue)
                z = self.z.view(B, S, self.Vp)[:, T + pos - 1, lo:hi]
                tok = pick(z, S * self.Vp, None, T + pos - 1)
            else:
                if pos == 0:
                    self._prefill(toks)                  # leaves k, v of the text positions in the cache
                # (position T - 1 is decoded again rather than read from the prefill's logits: every cached path then takes
                # every token through the same arithmetic)
                self.decode_step(toks[:, T + pos - 1].contiguous(), T + pos - 1, graph=decode_graph)
                if pos < k:
                    continue                             # teacher-forced: the prefix token is already in toks
                tok = pick(self._dec["z"], nv, bias, T + pos - 1)      # bf16 head output + bias, as the fused path draws
            toks[:, T + pos] = tok
        return result((toks[:R, T:] - lo).contiguous())

    @contextlib.contextmanager
    def kv_cache_as(self, kv_cache_dtype):
        """inside: the engine's cache type is kv_cache_dtype ("bf16", "fp8"; None: the default)"""
        prev, self.kv_cache_dtype = self.kv_cache_dtype, resolve_kv_cache_dtype(kv_cache_dtype)
        try:
            yield
        finally:
            self.kv_cache_dtype = prev

    def _kv_caches(self):
        """the per-layer key/value caches the decode step reads.  bf16: the [B*S, 3d] buffers -- the forward's own projection
        buffers, or under recompute_grad (one shared buffer) the sampler's, allocated once: L * B * S * 3d * 2 bytes.  fp8: per layer
        (data uint8 [B, S, 2, H, head_dim], scale fp32 [B, S, 2, H]), the sampler's, allocated once: L * B * S * (2d + 8H) bytes"""
        if self.kv_cache_dtype == "fp8":
            if self._kv8 is None:
                B, S, H = self.B, self.S, self.H
                self._kv8 = [(torch.empty(B, S, 2, H, self.hd, dtype=torch.uint8, device=self.dev),
                              torch.empty(B, S, 2, H, dtype=torch.float32, device=self.dev)) for _ in range(self.L)]
            return self._kv8
        if not self.recompute:
            return self.qkv
        if self._kv is None:
            self._kv = [torch.empty(self.M, 3 * self.d, dtype=torch.bfloat16, device=self.dev) for _ in range(self.L)]
        return self._kv

    def _prefill(self, toks):
        """evaluation forward over toks that leaves every layer's q | k | v in the decode caches (fp8: the forward keeps its own
        projection buffers -- one shared buffer under recompute_grad -- and quantises every layer's k | v out of them)"""
        shared = self.qkv
        if self.kv_cache_dtype == "fp8":
            self._kv8_out = self._kv_caches()
        else:
            self.qkv = self._kv_caches()                    # (the same list unless recompute_grad shares one buffer)
        self._shift_hist_out = self._shift_history()        # token_shift: the shift launches also write the history
        try:
            self.forward(toks, need_grad=False)
        finally:
            self.qkv = shared
            self._shift_hist_out = self._kv8_out = None

    def _shift_history(self):
        """token_shift: hist[l][site], bf16 [B, S, d/2] -- columns [0, d/2) of the output of norm_1 (site 0) / norm_2 (site 1) of
        block l at every position the sampler has passed, what later positions' shifts read.  The sampler's own, allocated once:
        L * B * S * d * 2 bytes, a third of the key/value caches.  Off: None."""
        if self.token_shift and self._shift_hist is None:
            self._shift_hist = [[torch.empty(self.B, self.S, self.d // 2, dtype=torch.bfloat16, device=self.dev) for _ in range(2)]
                                for _ in range(self.L)]
        return self._shift_hist

    def _decode_state(self):
        if self._dec is None:
            B, d = self.B, self.d
            b16 = dict(dtype=torch.bfloat16, device=self.dev)
            f32 = dict(dtype=torch.float32, device=self.dev)
            i32 = dict(dtype=torch.int32, device=self.dev)
            self._dec = dict(x=[torch.empty(B, d, **b16) for _ in range(2)], xn=torch.empty(B, d, **b16), o=torch.empty(B, d, **b16),
                             h=torch.empty(B, 4 * d, **b16), pre=torch.empty(B, self.F1, **b16) if self.ff_glu else None, st=[torch.empty(B, **f32) for _ in range(2)],
                             z=torch.empty(B, self.image_vocab_size, **b16), fresh=torch.empty(B, 3 * d, **b16),
                             tok=torch.empty(B, **i32), pos_i=torch.zeros(2, **i32),    # [position, scratch counter of the sampler]
                             logits=torch.empty(B, self.image_vocab_size, **f32),
                             params=torch.zeros(6, **i32), out=torch.zeros(B, self.S - self.T, **i32), logp=torch.zeros(B, **f32),
                             graphs={}, warm=set())
            if self.token_shift:
                self._dec["xs"] = torch.empty(B, d, **b16)       # the shifted row
        return self._dec

    def decode_step(self, tokens_at_pos: torch.Tensor, pos: int, graph: bool = True) -> torch.Tensor:
        """Incremental inference (reference hooks src/dalle_mtf/models.py:246-254,281-285): the hidden state of sequence
        position `pos` alone, given the tokens int32 [B] at that position and the key/value cache of positions < pos left by
        forward() / earlier decode steps in self.qkv[l] (under recompute_grad: in the sampler's caches, filled by its prefill).  Returns fp32 logits over the IMAGE vocabulary [B, image_vocab_size]
        (what predicts the token at pos + 1; the buffer is reused by the next call).

        graph=True: the ~90 launches of a step are a few microseconds of GPU work each, so the step is launch-bound when
        driven from the host; it is captured ONCE as a HIP graph and replayed for every position.  Nothing position-dependent
        is a by-value kernel argument: the position lives in device memory (pos_dev of dmi_embed_fwd -- the positional-embedding
        row -- and of dmi_attention_decode), and the QKV GEMM writes a fixed staging buffer that the attention kernel
        moves into cache row pos.  graph=False runs the same launches eagerly (the cross-check)."""
        B, S = self.B, self.S
        assert tokens_at_pos.shape == (B,) and tokens_at_pos.dtype == torch.int32 and 0 <= pos < S
        D = self._decode_state()
        D["tok"].copy_(tokens_at_pos)
        D["pos_i"][0:1].fill_(pos)
        self._run_decode(sample=False, graph=graph)
        return D["logits"]

    def _run_decode(self, sample, graph: bool):
        """sample: False (the decode_step body) or the draw variant (a Draw) -- one captured graph per variant and cache type: the
        draw node and the attention nodes differ.  The bf16 graphs are keyed by the variant alone, the fp8 ones by ("fp8", variant)."""
        D = self._dec
        key = sample if self.kv_cache_dtype == KV_DEFAULT else (self.kv_cache_dtype, sample)
        if not graph:
            self._decode_body(sample)
        elif key not in D["graphs"] and key not in D["warm"]:
            self._decode_body(sample)      # first step eager: lazily created views / copies come into being outside the capture
            D["warm"].add(key)
        else:
            if key not in D["graphs"]:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                # other host threads (input producer) stay free to call HIP; no finaliser runs inside the capture
                with _no_gc_in_capture(), torch.cuda.graph(g, capture_error_mode="thread_local"):
                    self._decode_body(sample)
                D["graphs"][key] = g       # (capture records, it does not execute: the replay below is the step)
            D["graphs"][key].replay()

    def _decode_body(self, sample=False):
        """the launches of one decode step; reads D[tok] and the position D[pos_i][0] from device memory.  sample=False: writes
        D[logits].  sample a Draw: draws the next token (settings in D[params]) into D[tok] and column pos - (T - 1) of D[out]
        (and D[logp], see _draw), then advances the position (inside the sampling kernel).
        B <= 32: LayerNorm rides in the prologue of the product that consumes it (dmi_ln_gemm_nt) -- 5 dependent launches per
        block instead of 7; a dependent launch costs ~7 us on this part, more than any of these kernels' work.
        token_shift: the two block LayerNorms take the unfused route with dmi_token_shift_decode between LayerNorm and product; it
        reads the neighbours' rows from the sampler's history and writes this position's (_shift_history)."""
        B, d, L, H, S = self.B, self.d, self.L, self.H, self.S
        D = self._dec
        x, x1, xn, o, h, st, z, fresh = D["x"][0], D["x"][1], D["xn"], D["o"], D["h"], D["st"], D["z"], D["fresh"]
        fuse_ln = B <= 32 and d <= 2048 and self.image_vocab_size % 16 == 0 and self.decode_fuse_ln

        hist = self._shift_history()

        def ln_dense(inp, ln, W, out, N, flags=0, bias=None, shift=None):       # out = LN(inp) . W^T (+ bias)(ReLU / GELU)
            g, b = self._w(ln + "/g"), self._w(ln + "/b")
            if hist is not None and shift is not None:   # token_shift, shift = (layer, site): the shift stands between LayerNorm and product
                dh.layernorm_fwd(inp, g, b, xn, st[0], st[1], B, d)
                dh.token_shift_decode(xn, hist[shift[0]][shift[1]], D["xs"], B, S, self.T, self.G, d, pos_dev=D["pos_i"])
                dh.gemm_nt(D["xs"], d, W, d, out, N, B, N, d, flags, bias=bias)
            elif fuse_ln:
                dh.ln_gemm_nt(inp, d, g, b, W, d, out, N, B, N, d, flags, bias=bias)
            else:
                dh.layernorm_fwd(inp, g, b, xn, st[0], st[1], B, d)
                dh.gemm_nt(xn, d, W, d, out, N, B, N, d, flags, bias=bias)

        act = dh.GEMM_GELU if self.activation == "gelu" else dh.GEMM_RELU
        caches = self._kv_caches()
        dh.embed_fwd(D["tok"], self._w("embedding/wte"), self._w("positional_embedding/wpe"), x, S, d, self.V,
                     pos_dev=D["pos_i"])                                  # every row takes wpe[pos]
        for l in range(L):
            p = f"layer_{l}/"
            cache = caches[l]                                          # bf16: [B*S, 3d], row b*S + pos <- q | k | v of this step
            ln_dense(x, p + "norm_1", self.tview(p + "attn/qkv"), fresh, 3 * d, shift=(l, 0))
            if self.qk_norm:                                           # normalised (and rotated at table row pos) before they enter the cache
                dh.qk_norm_decode(fresh, *self._qk_gains(l), B, S, H, self.hd, cs=self.rope_cs, pos_dev=D["pos_i"])
            elif self.rope_cs is not None:                             # q | k of the step at table row pos, before they enter the cache
                dh.rope_qk_decode(fresh, self.rope_cs, B, S, H, self.hd, pos_dev=D["pos_i"])
            self._attn_decode(l, cache, o, fresh, D["pos_i"])
            dh.gemm_nt(o, d, self.tview(p + "attn/o"), d, x1, d, B, d, d, dh.GEMM_BIAS | dh.GEMM_RESIDUAL,
                       bias=self._w(p + "attn/compute_output_bias/o_b"), residual=x)
            if self.ff_glu:    # [value | gate] into the [B, 8d] staging buffer with the bias only, then the gate: nothing depends on the position
                ln_dense(x1, p + "norm_2", self.tview(p + "mlp/mlp_linear_1/kernel"), D["pre"], self.F1, dh.GEMM_BIAS,
                         bias=self._w(p + "mlp/mlp_linear_1/bias"), shift=(l, 1))
                dh.glu_fwd(D["pre"], self.F1, h, 4 * d, B, 4 * d, self.activation)
            else:
                ln_dense(x1, p + "norm_2", self.tview(p + "mlp/mlp_linear_1/kernel"), h, 4 * d, dh.GEMM_BIAS | act,
                         bias=self._w(p + "mlp/mlp_linear_1/bias"), shift=(l, 1))
            dh.gemm_nt(h, 4 * d, self.tview(p + "mlp/mlp_linear_2/kernel"), 4 * d, x, d, B, d, 4 * d,
                       dh.GEMM_BIAS | dh.GEMM_RESIDUAL, bias=self._w(p + "mlp/mlp_linear_2/bias"), residual=x1)
        lo, nv = self.text_vocab_size, self.image_vocab_size
        Wt = self.tview("to_logits/linear_out/kernel")                 # [Vp, d]: rows lo .. lo + nv are the image vocabulary
        ln_dense(x, "to_logits/layer_norm", Wt[lo:lo + nv], z, nv)
        bias = self._w("to_logits/linear_out/bias")[lo:lo + nv]
        if sample:
            self._draw(sample, z, nv, bias, D["tok"], D["logp"], params_dev=D["params"], pos_dev=D["pos_i"], advance=True, out=D["out"],
                       out_col0=self.T - 1)
        else:
            dh.logits_f32(z, nv, bias, D["logits"], B, nv)       # "go to full precision for the logits" (models.py:394-395)

    def _draw(self, v, z, ldz, bias, next_tok, logp, top_p=1.0, scale=1.0, **kw):
        """launches the draw of variant v (a Draw) over the engine's B rows of head output z into next_tok; kw: the settings by
        value or in device memory (dalle_hip.sample_tokens).  v.nucleus: the nucleus kernel; v.logp: it adds the choice's
        log-probability to logp; v.guided: one token per pair of rows (b, B/2 + b) with the guided kernel, into both rows of
        next_tok and rows 0 .. B/2-1 of out / logp"""
        B, nv = self.B, self.image_vocab_size
        kw.update(token_offset=self.text_vocab_size, next_tok=next_tok)
        if v.nucleus:
            kw.update(top_p=top_p, logp=logp if v.logp else None)
        if v.guided:
            dh.sample_tokens_guided(z, ldz, bias, B // 2, nv, scale=scale, **kw)
        elif v.nucleus:
            dh.sample_tokens_p(z, ldz, bias, B, nv, **kw)
        else:
            dh.sample_tokens(z, ldz, bias, B, nv, **kw)

    # ------------------------------------------------------------------ backward
    def _gv(self, name):
        return self.view(self.g, name)

    # ---- weight gradients: dW = X^T dY (+ the bias gradient) as problem records in the form dh.gemm_tn_group takes
    def _wgrad_problems(self, l, dya, dyb):
        """block l's four weight gradients in the order of wgrad_shapes.  dya / dyb: the gradients of the FFN's and of the attention
        branch's output.  (X is [M, I], dY [M, J], both dense: the leading dimensions are I and J.)"""
        d, p, g = self.d, f"layer_{l}/", self._gv
        operands = ((self.h[l], dya, "mlp/mlp_linear_2/kernel", "mlp/mlp_linear_2/bias"),
                    (self.xn2[l], self._ffn1_grad_in(), "mlp/mlp_linear_1/kernel", "mlp/mlp_linear_1/bias"),
                    (self.o[l], dyb, "attn/o", "attn/compute_output_bias/o_b"),
                    (self.xn1[l], self.dqkv, "attn/qkv", None))
        return [dict(X=X, ldx=I, dY=dY, ldy=J, dW=g(p + w), I=I, J=J, ws=ws, **({"dbias": g(p + b)} if b else {}))
                for (X, dY, w, b), (I, J), ws in zip(operands, self.wgrad_shapes, self.ws_blk)]

    def _tn_launch(self, due, deferred=None):
        """one launch for the records in `due`: the grouped entry for several, dmi_gemm_tn for one.  deferred None: the slab
        reduces follow at once (the head's gradient, whose prefix of the flat buffer goes to the exchange first)."""
        if len(due) > 1:
            dh.gemm_tn_group(due, self.M, deferred=deferred)
        elif due:
            q = due[0]
            dh.gemm_tn(q["X"], q["ldx"], q["dY"], q["ldy"], q["dW"], self.M, q["I"], q["J"], q["ws"], dbias=q.get("dbias"),
                       bias_weights=q.get("bias_weights"), deferred=deferred)

    def _wgrad(self, probs, final):
        """launches those of a block's problems that are due once the operands of problem `final` are final: all four behind the
        last one (wgrad_group4), or the FFN's two each on its own and the attention pair (16 + 48 tiles fill the chip together)
        behind the last.  The operands of a problem stay untouched until its launch; the slab reduces of all four wait for the
        block's single reduce launch (self.deferred.run())."""
        if final == 3:
            due = probs if self.wgrad_group4 else probs[2:]
        else:
            due = [] if self.wgrad_group4 else [probs[final]]
        self._tn_launch(due, self.deferred)

    # ---- the input gradient into a LayerNorm
    def _d_o_chained(self):
        """norm_2's fused backward also forms the out-projection's input gradient d_o = dxb . Wo^T in the same launch -- not under
        residual dropout, where d_o = dyb . Wo^T reads the masked gradient"""
        return self.fuse_lnbwd and not self._drop_resid()

    def _ln_dgrad(self, idx, dres, dx):
        """dx = the gradient into the input of LayerNorm idx (2l: norm_1 of block l, 2l + 1: its norm_2, 2L: to_logits') + dres,
        and the LayerNorm's gain / bias gradients.  The gradient of its output is the product A . W^T of the layer that reads it
        (FFN-1: A = self.dh, gated self.dpre; QKV: A = self.dqkv); the head's is already in self.dxn.  fuse_lnbwd: product and LayerNorm backward
        in one pass (dmi_gemm_nt_lnbwd), chained with d_o for norm_2 (_d_o_chained); otherwise the product into self.dxn and
        dmi_layernorm_bwd.  The gain / bias partials are summed right away, or under lnb_batch by the next _flush_ln() -- the
        head's, which has no fused form, then joins the batch through a workspace of its own.  token_shift (never fused): the
        block LayerNorms' output gradient is the product shifted back, dmi_token_shift(inverse), from dxn into the scratch buffer."""
        M, d, L = self.M, self.d, self.L
        l, second = divmod(idx, 2)
        if idx == 2 * L:
            ln, x, (mean, rstd), A = "to_logits/layer_norm/", self.X[L], self.statf, None
        elif second:
            ln, x, (mean, rstd) = f"layer_{l}/norm_2/", self.x1[l], self.stats[l][2:]
            A, K, W = self._ffn1_grad_in(), self.F1, self._w(f"layer_{l}/mlp/mlp_linear_1/kernel")
        else:
            ln, x, (mean, rstd) = f"layer_{l}/norm_1/", self.X[l], self.stats[l][:2]
            A, K, W = self.dqkv, 3 * d, self._w(f"layer_{l}/attn/qkv")
        g, dg, db = self._w(ln + "g"), self._gv(ln + "g"), self._gv(ln + "b")
        if self.fuse_lnbwd and A is not None:
            kw = dict(B2=self._w(f"layer_{l}/attn/o"), ldb2=d, C2=self.d_o) if second and self._d_o_chained() else {}
            part = self.lnb_part[idx if self.lnb_batch else 0]
            now = {} if self.lnb_batch else dict(dg=dg, db=db)
            dh.gemm_nt_lnbwd(A, K, W, K, M, d, K, x, g, mean, rstd, dres, dx, part, **now, **kw)
            if self.lnb_batch:   # (finish_batch derives the number of partial rows from a row count: 32 rows per partial row)
                self._ln_pend.append((part, dg, db, 32 * dh.gemm_nt_lnbwd_parts(M)))
        elif A is None and self.lnb_batch:
            dh.layernorm_bwd(self.dxn, x, g, mean, rstd, dres, dx, None, None, self.ln_ws_final, M, d)
            self._ln_pend.append((self.ln_ws_final, dg, db, M))
        else:
            dy = self.dxn
            if A is not None:
                dh.gemm_nt(A, K, W, K, self.dxn, d, M, d, K)
                if self.token_shift:   # gradient w.r.t. the shifted rows -> w.r.t. the LayerNorm's output (the shift's transpose)
                    dy = self.shift_tmp
                    dh.token_shift(self.dxn, dy, M, self.S, self.T, self.G, d, inverse=True)
            dh.layernorm_bwd(dy, x, g, mean, rstd, dres, dx, dg, db, self.ws, M, d)

    def _flush_ln(self):
        """sums the queued gain / bias partials, 16 LayerNorms per launch"""
        while self._ln_pend:
            dh.layernorm_bwd_finish_batch(self._ln_pend[:16], self.d)
            del self._ln_pend[:16]

    def _launch_sort(self):
        main = torch.cuda.current_stream()
        self.sort_stream.wait_stream(main)
        with torch.cuda.stream(self.sort_stream):
            dh.sort_tokens(self.tokens, self.tok_sorted, self.tok_perm, self.M, self.V, self.sort_ws)
            self._sort_done = torch.cuda.Event()
            self._sort_done.record(self.sort_stream)

    def backward(self, allreduce=True):
        """Gradients of the last forward(need_grad=True) into the flat fp32 buffer.  With world_size > 1 every finished
        prefix of the buffer is handed to the exchange (src/dp.py: SUM all-reduce in <= 64 MB pieces on the side stream) --
        the explicit form of mtf's implicit all-reduce over the `data` mesh axis (src/model_fns.py:81-82,189)."""
        self._not_in_ema("backward")
        reserve = self.dp_reserve_cus if allreduce else 0
        if not reserve:
            return self._backward(allreduce)
        dh.set_option("reserve_cus", reserve)     # (read at launch time: applies to the launches enqueued inside the try)
        try:
            return self._backward(allreduce)
        finally:                                  # the option is process-global: never leave it set for later forwards / other engines
            dh.set_option("reserve_cus", 0)

    def _backward(self, allreduce):
        M, d, L, Vp = self.M, self.d, self.L, self.Vp
        E = self.z   # unnormalised dlogits: dlogits[m, :] = rowscale[m] * E[m, :]
        cuts = [0] + self.lay.ready_points

        def ready(i):   # g[cuts[i], cuts[i + 1]) is final on this stream: hand it to the exchange
            if allreduce:
                self.reducer.ready(cuts[i], cuts[i + 1])

        if self._sort_done is None:
            self._launch_sort()
        # head: dW = (rowscale * xnf)^T E, dbias = rowscale^T E, dxn = rowscale * (E W^T)
        self._tn_launch([dict(X=self.xs, ldx=d, dY=E, ldy=Vp, dW=self._gv("to_logits/linear_out/kernel"), I=d, J=Vp, ws=self.ws,
                              dbias=self._gv("to_logits/linear_out/bias"), bias_weights=self.rowscale_bf)])
        ready(0)
        # K = vocabulary: main-loop-bound -> 256x256 tiles, one 8-wave block per CU (the library picks that kernel for long-K
        # launches that fill whole residencies of the 256 CUs).  The rows of the whole residencies run unsplit; the rows of the
        # ragged last residency run with K split so that they also fill the chip (fp32 slabs, deterministic reduce).
        Wk = self._w("to_logits/linear_out/kernel")
        tn8 = (d + 255) // 256
        whole_rows = min(M, (((M + 255) // 256) * tn8 // 256) * 256 // tn8 * 256) if self.dgrad_tail_split else M
        if whole_rows in (0, M) or Vp < 8192:
            dh.gemm_nt(E, Vp, Wk, Vp, self.dxn, d, M, d, Vp, dh.GEMM_ROWSCALE, rowscale=self.rowscale)
        else:
            tail_rows = M - whole_rows
            tail_tiles = ((tail_rows + 255) // 256) * tn8
            ns = next((k for k in (2, 4, 8) if (tail_tiles * k) % 256 == 0 and Vp // k >= 4096), 2)
            dh.gemm_nt(E, Vp, Wk, Vp, self.dxn, d, whole_rows, d, Vp, dh.GEMM_ROWSCALE, rowscale=self.rowscale)
            dh.gemm_nt_splitk(E[whole_rows:], Vp, Wk, Vp, self.dxn[whole_rows:], tail_rows, d, Vp, ns, self.ws,
                              rowscale=self.rowscale[whole_rows:])
        dxa, dxb = self.dx
        self._ln_dgrad(2 * L, None, dxa)
        # residual dropout: the two branch outputs' gradients are the masked stream gradients (dya: dxa masked, dyb: dxb masked
        # after norm_2's backward); the unmasked dxa / dxb stay the residual pass-through
        drop = self._drop_resid()
        dya, dyb = self.dyd if drop else (dxa, dxb)
        for bi, l in enumerate(reversed(range(L))):
            p = f"layer_{l}/"
            if self.recompute:
                self._block_forward(l, rerun=True)
            probs = self._wgrad_problems(l, dya, dyb)
            # FFN
            if drop:
                dh.dropout_bwd(dxa, dya, M, d, *self.last_dropout[site_mlp(l)])
            self._wgrad(probs, 0)
            self._ffn2_dgrad(l, dya)
            self._wgrad(probs, 1)
            self._ln_dgrad(2 * l + 1, dxa, dxb)
            # attention
            if drop:
                dh.dropout_bwd(dxb, dyb, M, d, *self.last_dropout[site_attention(l)])
            if not self._d_o_chained():
                dh.gemm_nt(dyb, d, self._w(p + "attn/o"), d, self.d_o, d, M, d, d)
            self._attn_bwd(l)
            if self.qk_norm:   # gradient w.r.t. the normalised (and rotated) q, k -> w.r.t. the projection's output, and the gains' gradients
                dh.qk_norm_bwd(self.dqkv, self.qk_pre[l], *self._qk_gains(l), *self._qk_gains(l, self.g), self.ws, M, self.S, self.H,
                               self.hd, cs=self.rope_cs)
            elif self.rope_cs is not None:   # gradient w.r.t. the rotated q, k -> w.r.t. the projection's output (the rotation's transpose)
                dh.rope_qk(self.dqkv, self.rope_cs, M, self.S, self.H, self.hd, inverse=True)
            self._wgrad(probs, 3)
            self._ln_dgrad(2 * l, dxb, dxa)
            self.deferred.run()        # the block's seven slab reduces in one launch
            if allreduce and self.world > 1:
                self._flush_ln()       # the exchange takes this block's gradients now
            ready(1 + bi)
        # embeddings: positions visited in token-id order (sorted on the side stream during the forward)
        if self._sort_done is not None:
            torch.cuda.current_stream().wait_event(self._sort_done)
        self._embed_bwd(dxa)
        self._flush_ln()
        ready(L + 1)

    def wait_grads(self):
        self.reducer.finish()

    # ------------------------------------------------------------------ optimizer
    def learning_rate(self, step=None) -> float:
        """src/optimizers.py:46-76 (cosine/linear decay to 0.1*lr, linear warm-up)."""
        hp = self.hp
        step = self.global_step if step is None else step
        lr0 = hp["lr"]
        end = hp.get("lr_decay_end") or hp["train_steps"]
        decay = hp.get("lr_decay", "cosine") or "cosine"
        warm = hp.get("warmup_steps", 3000)
        warm = 3000 if warm is None else warm
        f32 = np.float32
        s = min(step, end)
        if decay == "linear":
            v = f32((lr0 - lr0 * 0.1) * (1.0 - s / end) + lr0 * 0.1)
        elif decay == "cosine":
            v = f32(lr0 * ((1.0 - 0.1) * 0.5 * (1.0 + math.cos(math.pi * s / end)) + 0.1))
        else:
            v = f32(lr0)
        if warm > 0 and step < warm:
            v = f32(v * f32(f32(step) / f32(warm)))
        return float(v)

    def optimizer_step(self):
        """the optimizer src/optimizers.py:78-99 selects, on the all-reduced gradients; refreshes the bf16 compute copies"""
        self.wait_grads()
        self._not_in_ema("optimizer_step")
        if self.optimizer == "adafactor":
            return self._adafactor_step()
        return self._adam_step()

    def _finish_step(self, lr):
        """behind either optimizer's launches: the weight average, the [out, in] compute copies (the optimizer kernel has
        written pb), the step count"""
        self._ema_update()
        self.refresh_compute_copies(cast=False)
        self.global_step += 1
        return lr

    def _adafactor_step(self):
        """clip_by_global_norm (src/optimizers.py:11-16, applied first, :100-103) + mtf.optimize.AdafactorOptimizer
        (src/optimizers.py:91-97) over every variable in six launches (dmi_adafactor_step); refreshes the bf16 compute copies."""
        hp = self.hp
        clip = hp.get("gradient_clipping", 1.0)
        lr = self.learning_rate()
        get = lambda k, dflt: dflt if hp.get(k) is None else float(hp[k])   # noqa: E731  (0.0 is a value, not "unset")
        if self._af_beta1() != 0.0 and self.m is None:   # beta_1 set after the state was allocated
            self.m = torch.zeros(self.lay.total, dtype=torch.float32, device=self.dev)
        dh.adafactor_step(self.af_table, len(self.af_vars), self.af_totals, self.p, self.g, self.m, self.af_slots, self.pb,
                          self.gnorm_sq, 0.0 if clip is None else float(clip), lr, get("weight_decay", 0.0), self._af_beta1(),
                          get("epsilon_1", 1e-30), get("epsilon_2", 1e-3), self.af_ws)
        return self._finish_step(lr)

    def _adam_step(self):
        """clip_by_global_norm (src/optimizers.py:11-16) + AdamWeightDecayOptimizer without bias correction
        (src/optimizers.py:82-89,154-177) on the all-reduced gradients; refreshes the bf16 compute copies."""
        hp = self.hp
        n = self.lay.total
        clip = hp.get("gradient_clipping", 1.0)
        lr = self.learning_rate()
        b1 = hp.get("beta_1") or 0.9
        b2 = hp.get("beta_2") or 0.999
        eps = hp.get("epsilon") or 1e-6
        wd = hp.get("weight_decay") or 0.0
        gn = None
        cl = 0.0
        if clip is not None:
            dh.sumsq(self.g, n, self.gnorm_sq, self.ws)
            gn, cl = self.gnorm_sq, float(clip)
        if not wd:
            dh.adam_step(self.p, self.g, self.m, self.v, self.pb, n, gn, cl, lr, b1, b2, eps, 0.0)
        else:
            for name, _ in self.lay.entries:
                o, k = self.lay.offset[name], _round_up(self.lay.numel(name), ALIGN)
                use = ("norm" not in name) and ("bias" not in name) and not name.endswith("o_b")
                dh.adam_step(self.p[o:o + k], self.g[o:o + k], self.m[o:o + k], self.v[o:o + k], self.pb[o:o + k], k, gn, cl,
                             lr, b1, b2, eps, wd if use else 0.0)
        return self._finish_step(lr)

    def train_step(self, tokens: torch.Tensor) -> torch.Tensor:
        """One optimizer step.  With hparams["num_microbatches"] = n > 1, `tokens` holds n micro-batches of B rows
        ([n*B, S]): gradients are accumulated locally and reduced once, and the loss is the sum of the micro-batch
        means / n (mtf.serialize_training_step as used at src/model_fns.py:156-166; src/dalle_mtf/models.py:356).  With loss
        weights set, self.loss_parts_acc accumulates the micro-batches' (text mean, image mean) / n the same way, and with
        "loss_ignore_padding" on self.text_kept_frac_acc their kept fractions / n (every micro-batch is normalised by its own
        counts: the step's loss is the mean of the masked means)."""
        self._not_in_ema("train_step")
        nmb = self.hp.get("num_microbatches", 1) or 1
        if nmb == 1:
            loss = self.forward(tokens, need_grad=True)
            self.backward()
            self.optimizer_step()
            return loss
        assert tokens.shape == (nmb * self.B, self.S), f"expected {nmb} micro-batches of {self.B} rows"
        if self.gacc is None:
            self.gacc = torch.empty_like(self.g)
        if self.loss_acc is None:         # (the model function creates the loss accumulators before the first step: its summaries hold them)
            self.loss_acc = torch.zeros_like(self.loss)
        self.loss_acc.zero_()
        if self.loss_parts is not None:
            if self.loss_parts_acc is None:
                self.loss_parts_acc = torch.zeros_like(self.loss_parts)
            self.loss_parts_acc.zero_()
        if self.text_kept_frac is not None:
            if self.text_kept_frac_acc is None:
                self.text_kept_frac_acc = torch.zeros_like(self.text_kept_frac)
            self.text_kept_frac_acc.zero_()
        for i in range(nmb):
            self._microbatch = i          # (keys the dropout masks: every micro-batch draws its own)
            loss = self.forward(tokens[i * self.B:(i + 1) * self.B], need_grad=True)
            self.loss_acc += loss
            if self.loss_parts is not None:
                self.loss_parts_acc.add_(self.loss_parts, alpha=1.0 / nmb)
            if self.text_kept_frac is not None:
                self.text_kept_frac_acc.add_(self.text_kept_frac, alpha=1.0 / nmb)
            self.backward(allreduce=False)
            if i == 0:
                self.gacc.copy_(self.g)
            else:
                dh.add_f32(self.gacc, self.g, self.lay.total)
        self._microbatch = 0
        self.g.copy_(self.gacc)
        self.reducer.ready(0, self.lay.total)
        self.optimizer_step()
        return self.loss_acc

    def grad_norm(self) -> float:
        return float(torch.sqrt(self.gnorm_sq).item())

    # ------------------------------------------------------------------ checkpoint
    def state_dict(self):
        sd = {"p": self.p.detach().cpu(), "global_step": self.global_step, "optimizer": self.optimizer, **checkpoint_entries(self.options)}
        for k in ("m", "v", "af_slots"):
            if getattr(self, k) is not None:
                sd[k] = getattr(self, k).detach().cpu()
        if self.ema is not None:       # the bf16 copy is recomputed on load
            sd["ema"] = self.ema.detach().cpu()
        return sd

    def load_state_dict(self, sd):
        written = sd.get("optimizer", "adam")   # checkpoints from before the optimizer was recorded are Adam's
        if written != self.optimizer:
            raise ValueError(f"checkpoint was written by the {written} optimizer; this run uses {self.optimizer}: "
                             "the optimizer state of one cannot continue the other")
        check_checkpoint(self.options, sd)
        self.p.copy_(sd["p"])
        for k in ("m", "v", "af_slots"):
            if getattr(self, k) is not None:
                if k not in sd:
                    raise ValueError(f"checkpoint has no {k!r} state for {self.optimizer} (beta_1 differs from the run's?)")
                getattr(self, k).copy_(sd[k])
        self.global_step = int(sd["global_step"])
        self.refresh_compute_copies(cast=True)
        if "ema" in sd:
            if self.ema is None:       # the run's config keeps no average: hold the checkpoint's for sampling, never update it
                self._alloc_ema()
            self.ema.copy_(sd["ema"])
            dh.cast_f32_bf16(self.ema, self.ema_b, self.lay.total)
        elif self.ema is not None:
            self._ema_from_p()
            if not self._ema_logged:
                self._ema_logged = True
                logging.getLogger("dalle_mtf_amd").info("checkpoint (step %d) carries no weight average: ema starts from its weights",
                                                        self.global_step)
