"""The model's options in one record: resolved from the config keys by the per-option modules (activations, loss_weights, ema,
dropout, rotary, token_shift, ff_glu, qk_norm), and what follows from the record alone -- the entries a checkpoint carries, the
check of a checkpoint against the run, the lines the model function logs and the fields generate.json reports.  Needs no
device."""
from typing import NamedTuple, Optional, Tuple

from .activations import resolve_activation
from .dropout import resolve_dropout
from .ema import resolve_ema
from .ff_glu import ffn1_width, resolve_ff_glu
from .loss_weights import resolve_loss_weights
from .qk_norm import resolve_qk_norm
from .rotary import DEFAULT_BASE, resolve_rotary
from .token_shift import grid_side, resolve_token_shift


class Options(NamedTuple):
    # the model: a checkpoint must match these
    activation: str                 # "relu" | "gelu", the FFN's hidden layer (reference src/dalle_mtf/models.py:317-324)
    rotary: Optional[str]           # "1d" | "axial" | None
    rotary_base: float
    token_shift: bool               # half of every position's channels come from its neighbours, behind norm_1 and norm_2
    ff_glu: bool                    # the gated FFN, h = value * act(gate) from an FFN-1 of width 8d
    qk_norm: bool                   # q and k RMS-normalised per head with learned gains behind the QKV product
    # training: not part of the checkpoint check
    loss_weights: Optional[Tuple[float, float]]    # (text, image); None: the reference's plain mean
    ema_decay: Optional[float]      # None: no weight average
    ema_eval: bool
    embed_thresh: int               # the dropout rates as 16-bit thresholds (0: off)
    resid_thresh: int
    dropout_seed: int


def resolve_options(params, n_embd, text_seq_len, image_seq_len, activation_fn=None):
    """every option from the config keys, each by its module's resolver; the first bad key (in this order) raises its error"""
    activation = resolve_activation(activation_fn, params)
    loss_weights = resolve_loss_weights(params, text_seq_len)
    ema_decay, ema_eval = resolve_ema(params)
    embed_thresh, resid_thresh, dropout_seed = resolve_dropout(params)
    rotary, rotary_base = resolve_rotary(params, image_seq_len)        # "axial" needs a square image grid
    token_shift = resolve_token_shift(params, n_embd, image_seq_len)   # needs a square image grid and n_embd % 32 == 0
    return Options(activation, rotary, rotary_base, token_shift, resolve_ff_glu(params), resolve_qk_norm(params),
                   loss_weights, ema_decay, ema_eval, embed_thresh, resid_thresh, dropout_seed)


def checkpoint_entries(opt):
    """what a checkpoint records of the model; a checkpoint without a key is a model with that option off"""
    sd = {"activation_fn": opt.activation}
    if opt.rotary is not None:
        sd["rotary_emb"], sd["rotary_base"] = opt.rotary, opt.rotary_base
    sd.update({k: True for k in ("token_shift", "ff_glu", "qk_norm") if getattr(opt, k)})
    return sd


# option -> (how a message names it on, how off)
_SWITCHES = (("token_shift", ("token_shift on", "no token shift")),
             ("ff_glu", ("ff_glu on (the gated FFN)", "ff_glu off (the plain FFN)")),
             ("qk_norm", ("qk_norm on (normalised q and k with learned gains)", "qk_norm off (plain q and k)")))


def check_checkpoint(opt, sd):
    """ValueError when the state dict sd was written by another model than opt's (checkpoints from before a key was recorded:
    a ReLU model, the option off)"""
    def refuse(theirs, mine):
        raise ValueError(f"checkpoint was written by a {theirs}; this run uses {mine}: the weights of one do not compute the other")

    act = sd.get("activation_fn", "relu")
    if act != opt.activation:
        refuse(f"{act} model", f"activation_fn {opt.activation!r}")
    rot = (sd.get("rotary_emb"), float(sd.get("rotary_base", DEFAULT_BASE)) if sd.get("rotary_emb") is not None else None)
    mine = (opt.rotary, opt.rotary_base if opt.rotary is not None else None)
    if rot != mine:
        say = lambda r: "no rotary embeddings" if r[0] is None else f"rotary_emb {r[0]!r} (rotary_base {r[1]:g})"   # noqa: E731
        refuse(f"model with {say(rot)}", say(mine))
    for key, (on, off) in _SWITCHES:
        theirs = bool(sd.get(key, False))
        if theirs != getattr(opt, key):
            refuse(f"model with {on if theirs else off}", off if theirs else on)


def option_log_lines(opt, n_embd, n_heads, text_seq_len, image_seq_len):
    """the lines the model function logs about the options that are on (it puts the mode in front of each)"""
    lines = []
    if opt.loss_weights is not None:
        lines.append("loss weights: text %g, image %g -> loss = (%g * mean_text + %g * mean_image) / %g over %d text and %d image positions"
                     % (*opt.loss_weights, *opt.loss_weights, sum(opt.loss_weights), text_seq_len - 1, image_seq_len + 1))
    if opt.ema_decay is not None:
        lines.append("weight EMA: ema_decay %g (decay at step t = min(%g, (1 + t) / (10 + t))), evaluation from the %s weights"
                     % (opt.ema_decay, opt.ema_decay, "averaged" if opt.ema_eval else "raw"))
    if opt.rotary is not None:
        lines.append("rotary embeddings: %s, base %g (in addition to the learned positions)" % (opt.rotary, opt.rotary_base))
    if opt.token_shift:
        G = grid_side(image_seq_len)
        lines.append("token shift: on (behind norm_1 and norm_2 of every block, %d x %d image grid)" % (G, G))
    if opt.ff_glu:
        lines.append("gated feed-forward: on (%s, mlp_linear_1 is [%d, %d])"
                     % ("GEGLU" if opt.activation == "gelu" else "ReGLU", n_embd, ffn1_width(n_embd, True)))
    if opt.qk_norm:
        hd = n_embd // n_heads
        lines.append("QK normalisation: on (RMS per head over %d channels, eps 1e-6, gains [%d] per layer)" % (hd, hd))
    return lines


def report(opt):
    """the options as generate.json reports them"""
    return dict(rotary_emb=opt.rotary, rotary_base=opt.rotary_base if opt.rotary is not None else None,
                token_shift=opt.token_shift, ff_glu=opt.ff_glu, qk_norm=opt.qk_norm)
