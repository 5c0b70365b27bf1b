"""Vector-quantised bottleneck of the discrete VAE: the config keys "quantizer" and "vq_commitment" (DESIGN.md §4 "VAE: vector
quantisation").  Host arithmetic only: nothing here needs a device.

With "quantizer": "vq" every encoder vector X[m] is replaced by its nearest code (column idx[m] of codebook/codebook), the decoder
runs on that code with a straight-through gradient, and
    loss = recon + (1 + beta) Lq,    Lq = mean over the M positions and D channels of (X[m] - code)^2,
the codebook loss (weight 1, gradient to the codebook alone) and the commitment loss (weight beta = "vq_commitment", gradient to
the encoder alone) having the same value.  No temperature, no noise.  "gumbel", unset and null: the reference's Gumbel-softmax
bottleneck, on the launches it always ran on."""
import math
from collections import namedtuple

import numpy as np

KEYS = ("quantizer", "vq_commitment")
QUANTIZERS = ("gumbel", "vq")
DEFAULT_COMMITMENT = 0.25

VaeVqOptions = namedtuple("VaeVqOptions", "quantizer vq_commitment")

STAT_SCALARS = ("loss_recon", "loss_vq", "perplexity_hard", "codes_used_frac")


def _is_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def resolve_vq_options(params):
    """VaeVqOptions(quantizer "gumbel" or "vq", vq_commitment float or None) from the config keys.  quantizer: "gumbel", unset or
    None = off; "vq" = on.  vq_commitment: a finite number >= 0, only with "vq" (default 0.25; None when off).  With "vq" a
    kl_loss_weight > 0 or a kl_anneal_steps is refused: there is no categorical posterior to regularise.  Anything else raises
    ValueError naming the key."""
    params = params or {}
    q = params.get("quantizer")
    if q is None:
        q = "gumbel"
    if not isinstance(q, str) or q not in QUANTIZERS:
        raise ValueError(f"config key quantizer: expected one of {', '.join(repr(v) for v in QUANTIZERS)} or null (got {q!r})")
    b = params.get("vq_commitment")
    if b is not None:
        if not _is_number(b) or not math.isfinite(b) or b < 0:
            raise ValueError(f"config key vq_commitment: expected a finite number >= 0 (got {b!r})")
        if q != "vq":
            raise ValueError('config key vq_commitment: needs "quantizer": "vq" (the Gumbel bottleneck has no commitment loss)')
    if q != "vq":
        return VaeVqOptions("gumbel", None)
    w = params.get("kl_loss_weight")
    if w is not None and not (_is_number(w) and float(w) == 0.0):
        raise ValueError('config key kl_loss_weight: not with "quantizer": "vq" (there is no categorical posterior to regularise)')
    if params.get("kl_anneal_steps") is not None:
        raise ValueError('config key kl_anneal_steps: not with "quantizer": "vq" (there is no KL term to ramp)')
    return VaeVqOptions("vq", DEFAULT_COMMITMENT if b is None else float(b))


def check_checkpoint(model_quantizer, sd):
    """a checkpoint carries "quantizer": "vq" only when it was trained with it (a missing key means Gumbel); the model that loads it
    must have been built with the same one"""
    ck = sd.get("quantizer") if isinstance(sd, dict) else None
    ck = "gumbel" if ck is None else ck
    if ck != model_quantizer:
        raise ValueError(f"checkpoint was trained with quantizer = {ck!r} but the model is built with quantizer = {model_quantizer!r}: "
                         f'set the VAE config key "quantizer" to {ck!r} (the codebook means something else under the other one)')


def vq_log_lines(opt, num_tokens, grid, n_hid):
    """the line the model function logs when the quantiser is on (it puts the mode in front)"""
    if opt.quantizer != "vq":
        return []
    return ["vector quantisation: quantizer vq, vq_commitment %g -> loss = recon + (1 + %g) * mean over %d x %d positions x %d channels of "
            "(x_enc - nearest of %d codes)^2, straight-through decoder gradient; temperature and Gumbel noise are ignored; %s with "
            "every summary and evaluation" % (opt.vq_commitment, opt.vq_commitment, grid, grid, n_hid, num_tokens, ", ".join(STAT_SCALARS))]
