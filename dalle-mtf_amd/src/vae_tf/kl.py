"""KL term and codebook statistics of the discrete VAE: the config keys "kl_loss_weight", "kl_anneal_steps" and "codebook_stats"
(DESIGN.md §4 "VAE: KL term and codebook statistics").  Host arithmetic only: nothing here needs a device.

The reference trains its dVAE on the bare reconstruction loss mean((img - out)^2) (src/vae_tf/models.py:180-183).  With a weight
beta > 0 the loss becomes
    loss = recon + beta_t * KL,    KL = mean over the M = B g g positions of KL(q(z|x) || uniform) in nats,
    beta_t = beta * min(1, step / kl_anneal_steps)      (beta when kl_anneal_steps is unset),
q the softmax of the codebook logits without noise or temperature.  dalle-pytorch's kl_div_loss_weight w (sum over positions,
mean over images) is beta = w g^2.  All keys absent: the reference's loss, on the launches it always ran on."""
import math
from collections import namedtuple

import numpy as np

KEYS = ("kl_loss_weight", "kl_anneal_steps", "codebook_stats")

VaeKlOptions = namedtuple("VaeKlOptions", "kl_loss_weight kl_anneal_steps codebook_stats")


def _is_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def resolve_kl_options(params):
    """VaeKlOptions(kl_loss_weight float (0.0 = off), kl_anneal_steps int or None, codebook_stats bool) from the three config keys.
    kl_loss_weight: finite, >= 0 (unset / None / 0 = off); kl_anneal_steps: a positive int, only with a weight > 0; codebook_stats:
    a bool.  Anything else raises ValueError naming the key."""
    params = params or {}
    w = params.get("kl_loss_weight")
    if w is None:
        w = 0.0
    if not _is_number(w) or not math.isfinite(w) or w < 0:
        raise ValueError(f"config key kl_loss_weight: expected a finite number >= 0 (got {w!r})")
    n = params.get("kl_anneal_steps")
    if n is not None:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n <= 0:
            raise ValueError(f"config key kl_anneal_steps: expected a positive integer (got {n!r})")
        if float(w) == 0.0:
            raise ValueError("config key kl_anneal_steps: needs kl_loss_weight > 0 (there is no KL term to ramp)")
        n = int(n)
    s = params.get("codebook_stats")
    if s is None:
        s = False
    if not isinstance(s, (bool, np.bool_)):
        raise ValueError(f"config key codebook_stats: expected true or false (got {s!r})")
    return VaeKlOptions(float(w), n, bool(s))


def kl_weight_at(step, kl_loss_weight, kl_anneal_steps=None):
    """beta_t = beta * min(1, step / kl_anneal_steps); beta when kl_anneal_steps is unset"""
    if not kl_anneal_steps:
        return float(kl_loss_weight)
    return float(kl_loss_weight) * min(1.0, float(step) / float(kl_anneal_steps))


def _perplexity(w):
    """exp(H(w / sum w)) in float64; a zero weight contributes 0"""
    w = np.asarray(w, np.float64)
    tot = w.sum()
    if not tot > 0:
        return float("nan")
    p = w / tot
    nz = p > 0
    return float(np.exp(-(p[nz] * np.log(p[nz])).sum()))


def usage_stats(qsum, counts, M):
    """the codebook statistics from qsum[k] = sum_m q[m, k] and counts[k] = #{m : index[m] == k} over M rows:
    perplexity_soft = exp(H(qsum / M)), perplexity_hard = exp(H(counts / M)), codes_used = #{counts > 0}, codes_used_frac"""
    counts = np.asarray(counts)
    T = int(counts.shape[0])
    used = int((counts > 0).sum())
    return dict(perplexity_soft=_perplexity(qsum), perplexity_hard=_perplexity(counts), codes_used=used, codes_used_frac=used / T)


STAT_SCALARS = ("loss_recon", "loss_kl", "kl_weight", "perplexity_soft", "perplexity_hard", "codes_used_frac")


def kl_log_lines(opt, num_tokens, grid):
    """the lines the model function logs about the keys that are on (it puts the mode in front of each)"""
    if opt.kl_loss_weight > 0:
        ramp = "constant" if opt.kl_anneal_steps is None else "ramped linearly from 0 over the first %d steps" % opt.kl_anneal_steps
        return ["KL term: kl_loss_weight %g (%s) -> loss = recon + beta_t * mean over %d x %d positions of KL(q || uniform over %d codes) "
                "in nats (dalle-pytorch's kl_div_loss_weight would be %g); codebook statistics with every summary and evaluation"
                % (opt.kl_loss_weight, ramp, grid, grid, num_tokens, opt.kl_loss_weight / (grid * grid))]
    if opt.codebook_stats:
        return ["codebook statistics: on (%s with every summary and evaluation; no KL term in the loss)" % ", ".join(STAT_SCALARS)]
    return []
