"""EMA codebook updates and dead-code restarts for the vector-quantised bottleneck: the config keys "vq_ema_decay",
"vq_restart_after" and "vq_restart_seed" (DESIGN.md §4 "VAE: EMA codebook and restarts").  Host arithmetic only: nothing here needs a
device.

With "vq_ema_decay": gamma the codebook is no longer trained by its gradient.  Per code k the model keeps N[k] (fp32), S[k][0..D)
(fp32) and idle[k] (int32); a training step takes its cluster sums n[k] = #{m : idx[m] = k}, s[k] = sum_{idx[m]=k} x_enc[m] and sets,
with g = fp32(gamma) and w = fp32(1 - gamma),
    n[k] > 0:  N' = g N + w n,  S' = g S + w s,  C[:,k] = S' / N',  idle = 0
    n[k] = 0:  N' = g N,        S' = g S,        C[:,k] unchanged,   idle += 1
so a code nobody picks neither drifts nor divides by a vanishing N.  With "vq_restart_after": R every code with idle >= R is then
re-seeded from an encoder row of the step, m_k = splitmix64(splitmix64(splitmix64(seed) ^ step) + k) mod M: C[:,k] = x_enc[m_k],
N = 1, S[k] = C[:,k], idle = 0.  Two dead codes may draw the same row; the arg-max's tie-break (lowest index wins) then leaves one of
them idle and it is re-seeded again R steps on.  The loss becomes recon + beta Lq (commitment only)."""
import math
from collections import namedtuple

import numpy as np

KEYS = ("vq_ema_decay", "vq_restart_after", "vq_restart_seed")

VaeVqEmaOptions = namedtuple("VaeVqEmaOptions", "vq_ema_decay vq_restart_after vq_restart_seed")
OFF = VaeVqEmaOptions(None, 0, 0)

EMA_STAT_SCALARS = ("vq_restarts", "codes_idle")     # joined to vq.STAT_SCALARS when the EMA codebook is on
STATE_KEYS = ("N", "S", "idle", "restarts")


def _is_number(v):
    return not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def resolve_vq_ema_options(params, world=1):
    """VaeVqEmaOptions(vq_ema_decay float or None, vq_restart_after int (0 = off), vq_restart_seed int) from the config keys.
    vq_ema_decay: a finite number with 0 < gamma < 1, only with "quantizer": "vq"; unset or None = off.  vq_restart_after: an int >= 1
    (bools refused), only with vq_ema_decay; unset, None or 0 = off.  vq_restart_seed: an int (default 0), only with vq_restart_after.
    vq_ema_decay with data-parallel training (world > 1) is refused: the cluster counts have no slot in the gradient exchange.
    Anything else raises ValueError naming the key."""
    params = params or {}
    g, R, seed = params.get("vq_ema_decay"), params.get("vq_restart_after"), params.get("vq_restart_seed")
    if g is not None:
        if not _is_number(g) or not math.isfinite(g) or not 0.0 < float(g) < 1.0:
            raise ValueError(f"config key vq_ema_decay: expected a finite number with 0 < decay < 1, or null (got {g!r})")
        q = params.get("quantizer")
        if q != "vq":
            raise ValueError(f'config key vq_ema_decay: needs "quantizer": "vq" (got quantizer = {q!r}; only a vector-quantised '
                             f"codebook has clusters to average)")
        if world > 1:
            raise ValueError(f"config key vq_ema_decay: not with data-parallel training (world = {world}): the cluster counts and sums "
                             f"have no slot in the gradient exchange")
    if R is not None:
        if not _is_int(R) or R < 0:
            raise ValueError(f"config key vq_restart_after: expected an int >= 1, or 0 / null for off (got {R!r})")
        if R > 0 and g is None:
            raise ValueError('config key vq_restart_after: needs "vq_ema_decay" (restarts without the EMA codebook are not built)')
    R = int(R or 0)
    if seed is not None:
        if not _is_int(seed):
            raise ValueError(f"config key vq_restart_seed: expected an int (got {seed!r})")
        if R == 0:
            raise ValueError('config key vq_restart_seed: needs "vq_restart_after" (nothing else draws from it)')
    if g is None:
        return OFF
    return VaeVqEmaOptions(float(g), R, int(seed or 0))


def check_checkpoint(model_decay, sd):
    """a checkpoint carries "vq_codebook": "ema" (and its state "vq_ema") only when it was trained with the EMA codebook; the model
    that loads it must have been built the same way"""
    ck = isinstance(sd, dict) and sd.get("vq_codebook") == "ema"
    if ck and model_decay is None:
        raise ValueError('checkpoint was trained with an EMA codebook but the model is built without vq_ema_decay: set the VAE config '
                         'key "vq_ema_decay" (the checkpoint\'s Adam moments of the codebook are zero and its cluster state would be lost)')
    if not ck and model_decay is not None:
        raise ValueError(f"checkpoint was trained with a gradient-trained codebook but the model is built with vq_ema_decay = "
                         f'{model_decay!r}: unset the VAE config key "vq_ema_decay" (the checkpoint has no cluster state N, S)')


def vq_ema_log_lines(opt, num_tokens):
    """the line the model function logs when the keys are on (it puts the mode in front)"""
    if opt.vq_ema_decay is None:
        return []
    tail = ("codes idle for %d steps are re-seeded from an encoder row (vq_restart_seed %d)" % (opt.vq_restart_after, opt.vq_restart_seed)
            if opt.vq_restart_after else "no restarts")
    return ["EMA codebook: vq_ema_decay %g over %d codes, loss = recon + vq_commitment * Lq, no codebook gradient; %s; %s with every "
            "summary and evaluation" % (opt.vq_ema_decay, num_tokens, tail, ", ".join(EMA_STAT_SCALARS))]
