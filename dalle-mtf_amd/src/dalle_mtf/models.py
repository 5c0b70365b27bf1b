"""DALLE -- same constructor / forward surface as the reference class (src/dalle_mtf/models.py:141-416),
re-hosted on the MI355X engine (hand-written HIP kernels behind libdalle_hip's C ABI)."""
from collections import defaultdict

import torch

import numpy as np

from .engine import DalleEngine
from .layout import ParamLayout
from .loss_mask import resolve_loss_ignore_padding
from .masks import layer_masks
from .ops import get_variable_dtype
from .options import resolve_options


def _causal(S):
    return np.tril(np.ones((S, S), dtype=bool))


class DALLE:
    def __init__(self, n_embd, text_vocab_size=12800, image_vocab_size=512, text_seq_len=256, image_seq_len=1024,
                 n_layers=6, n_heads=8, batch_size=32, bf_16=True, attn_mask=None, mode="train",
                 is_incremental_inference=False, context=None, loss_fn=None, params=None, eos_token_id=None,
                 activation_fn=None, device="cuda", process_group=None, world_size=1, global_batch_size=None, comm=None):
        self.n_embd = n_embd
        self.text_vocab_size = text_vocab_size
        self.image_vocab_size = image_vocab_size
        self.text_seq_len = text_seq_len
        self.image_seq_len = image_seq_len
        self.total_seq_dim = text_seq_len + image_seq_len
        self.n_layers = n_layers
        self.n_heads = n_heads
        self.total_tokens = text_vocab_size + image_vocab_size + 1  # extra for EOS (reference :157)
        self.eos_token_id = self.total_tokens - 1 if eos_token_id is None else eos_token_id
        self.bf_16 = bf_16
        self.variable_dtype = get_variable_dtype(bf_16)
        if not bf_16:
            # the reference's shipped configs/dalle_example.json has "bf_16": false = fp32 activations; the MI355X kernels keep fp32
            # masters / optimizer state but ALWAYS compute activations in bf16 with fp32 accumulation (stated
            # deviation): say so instead of silently running narrower arithmetic than the reference would
            import warnings
            warnings.warn("DALLE(bf_16=False): fp32 master weights and optimizer state are kept, but the MI355X kernels compute "
                          "activations in bf16 with fp32 accumulation -- narrower than the reference's fp32 activations for this "
                          "setting (loss agrees to ~1e-5 relative, gradients to a few percent per tensor; DESIGN.md §2)", stacklevel=2)
        self.mode = mode
        self.batch_size = batch_size
        if is_incremental_inference or context is not None:
            raise NotImplementedError("incremental inference is unfinished upstream (predict raises NotImplementedError, model_fns.py:135)")
        if loss_fn is not None:
            raise NotImplementedError("custom loss_fn: the kernels implement softmax cross-entropy (the reference default)")
        params = {} if params is None else params
        self.params = defaultdict(lambda: None, params)
        # the options (dalle_mtf.options), checked here, before any device work.  activation_fn (reference models.py:317-324, the
        # FFN's hidden layer): "relu" | "gelu" | None -> config key "activation_fn" -> "relu"
        self.options = opt = resolve_options(params, n_embd, text_seq_len, image_seq_len, activation_fn=activation_fn)
        self.activation_fn, self.rotary_emb, self.rotary_base = opt.activation, opt.rotary, opt.rotary_base
        self.token_shift, self.ff_glu, self.qk_norm = opt.token_shift, opt.ff_glu, opt.qk_norm
        # "loss_ignore_padding" (dalle_mtf.loss_mask): a training setting kept beside the options, checked here too
        self.loss_ignore_padding, self.loss_pad_id = resolve_loss_ignore_padding(params, text_seq_len, text_vocab_size)
        if self.params.get("attention_dropout"):
            raise NotImplementedError("attention_dropout > 0 is not supported: embed_dropout and residual_dropout are; dropout of "
                                      "the attention weights would live inside the attention kernels (all shipped configs use 0)")
        if (self.params.get("scale_type") or "scale_by_depth") != "scale_by_depth":
            raise NotImplementedError("scale_type other than scale_by_depth")
        # attn_mask (reference models.py:221-227, the attention bias at :292-299): a bool [S, S] mask, an additive float mask (0 or
        # <= -1e9), a pattern name (dalle_mtf.masks), or a list of n_layers of these; else the config key "attention_pattern" (a
        # name or a list of n_layers names).  Both absent: the causal kernels, unchanged.
        spec = attn_mask
        if spec is None and self.params.get("attention_pattern") is not None:
            spec = self.params["attention_pattern"]
            if not (isinstance(spec, str) or (isinstance(spec, (list, tuple)) and all(isinstance(x, str) for x in spec))):
                raise ValueError(f"config key attention_pattern: expected a pattern name or a list of {n_layers} names (got {spec!r})")
        attn_masks = None
        if spec is not None:
            attn_masks = layer_masks(spec, n_layers, text_seq_len, image_seq_len)
            causal = _causal(self.total_seq_dim)
            if all(np.array_equal(m, causal) for m in attn_masks):
                attn_masks = None
        self.engine = DalleEngine(n_embd, n_layers, n_heads, text_vocab_size, image_vocab_size, text_seq_len,
                                  image_seq_len, batch_size, global_batch_size=global_batch_size,
                                  eos_token_id=eos_token_id, hparams=dict(self.params, activation_fn=self.activation_fn), device=device,
                                  process_group=process_group, world_size=world_size, comm=comm, attn_masks=attn_masks)
        self.dimensions = {"embed_dim": n_embd, "final_vocab_dim": self.total_tokens, "total_seq_dim": self.total_seq_dim,
                           "heads_dim": n_heads, "kv_dim": n_embd // n_heads, "batch_dim": batch_size}

    def variables(self):
        """name -> shape under the reference's checkpoint names."""
        lay = ParamLayout(self.n_embd, self.n_layers, self.n_heads, self.total_tokens, self.total_seq_dim,
                          ff_glu=self.options.ff_glu, qk_norm=self.options.qk_norm)
        return {name: shape for name, shape, _, _ in lay.reference_variables()}

    def sample(self, text_tokens, vae=None, temperature=1.0, top_k=0, seed=0, top_p=1.0, image_prefix=None, return_logprobs=False,
               guidance_scale=1.0, uncond_text=None, weights=None, kv_cache_dtype=None):
        """text ids [B, text_seq_len] -> image-token ids [B, image_seq_len] (and the decoded images when a DiscreteVAE is
        given): the generation path the reference leaves unfinished (model_fns.py:135-136).  top_p < 1: nucleus filter after
        top-k; image_prefix int [B, k]: complete images from their first k tokens; return_logprobs: also the model's
        log-likelihood of each sample, fp32 [B] (DalleEngine.sample_image_tokens).  guidance_scale != 1 / uncond_text:
        classifier-free guidance -- text_tokens (and image_prefix) are [B / 2, ...], the other half of the batch carries
        uncond_text (default: the null caption), and B / 2 rows come back.  weights: "ema" samples from the weight average
        (config key "ema_decay"), "raw" from the raw iterate, None from the average when the engine has one; "ema" without an
        average raises ValueError.  kv_cache_dtype: "bf16" (None: the default) or "fp8", the sampler's key/value cache type
        (dalle_mtf.kv_cache); anything else raises ValueError.  Returns toks, (toks, images), (toks, logp) or
        (toks, images, logp)."""
        res = self.engine.sample_image_tokens(text_tokens, temperature=temperature, top_k=top_k, seed=seed, top_p=top_p,
                                              image_prefix=image_prefix, return_logprobs=return_logprobs,
                                              guidance_scale=guidance_scale, uncond_text=uncond_text, weights=weights,
                                              kv_cache_dtype=kv_cache_dtype)
        toks, logp = res if return_logprobs else (res, None)
        out = (toks, vae.decode_tokens(toks)) if vae is not None else (toks,)
        if return_logprobs:
            out = out + (logp,)
        return out if len(out) > 1 else out[0]

    def forward(self, features, return_loss=True, return_logits=False):
        """features["tokens"]: int32 [B, S] device tensor.  Returns (loss, loss_batch[, logits]) like the
        reference (models.py:397-416); with return_loss=False returns the fp32 logits only.  With loss weights set, loss is
        the weighted loss; loss_batch stays the unweighted per-position NLL.  Dropout applies to the training forward only:
        return_logits=True (or return_loss=False) runs the evaluation path, undropped, in train mode too."""
        tokens = features["tokens"] if isinstance(features, dict) else features
        tokens = tokens.to(device=self.engine.dev, dtype=torch.int32)
        need_grad = self.mode == "train" and return_loss and not return_logits
        loss = self.engine.forward(tokens, need_grad=need_grad)
        if not return_loss:
            return self.engine.logits()
        loss_batch = self.engine.loss_rows.view(self.batch_size, self.total_seq_dim)
        if return_logits:
            return loss[0], loss_batch, self.engine.logits()
        return loss[0], loss_batch
