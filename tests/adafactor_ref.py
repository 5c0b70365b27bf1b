"""Float64 restatement of mtf.optimize.AdafactorOptimizer as src/optimizers.py:91-97 builds it (test infrastructure only).

[MTF-RECALL] The per-variable update is restated from mesh-tensorflow 0.1.18's optimize.py from memory, as SURVEY.md Appendix A
restates the other third-party primitives: no mesh-tensorflow is available to check it against.  Defaults kept from mtf:
multiply_by_parameter_scale=True, clipping_threshold=1.0, factored=True, min_dim_size_to_factor=128.

    g2    = g*g + eps1
    scale = lr * max(rms(w), eps2)
    factored:   vr = decay*vr + (1-decay)*mean_over_d0(g2)   (indexed along d1)
                vc = decay*vc + (1-decay)*mean_over_d1(g2)   (indexed along d0)
                x  = g * rsqrt(vr / mean(vr)) * rsqrt(vc)
    otherwise:  v  = decay*v + (1-decay)*g2;   x = g * rsqrt(v)
    x = x / max(1, rms(x) / 1.0);  u = scale * x
    beta1 != 0: m = beta1*m + (1-beta1)*u;  u = m
    w -= u

Slots are zero-initialised and named <var>_slot_vr, _slot_vc, _slot_v, _slot_m.  train() runs the reference's train step with
it: oracle.dalle_oracle.loss_and_grads -> clip_by_global_norm -> learning_rate -> this update."""
from collections import OrderedDict

import numpy as np

from oracle import dalle_oracle as do

MIN_DIM_SIZE_TO_FACTOR = 128
CLIPPING_THRESHOLD = 1.0


def hyper_parameters(params):
    """get_optimizer's argument mapping (src/optimizers.py:92-97): weight_decay is the SECOND-MOMENT DECAY RATE"""
    return dict(decay=params.get("weight_decay", 0.0), beta1=params.get("beta_1", 0.9), eps1=params.get("epsilon_1", 1e-30),
                eps2=params.get("epsilon_2", 1e-3))


def factored_dims(shape):
    """(d0, d1) axes or None: dims sorted by size, descending and stable; None below rank 2 or when d1 < 128"""
    if len(shape) < 2:
        return None
    order = sorted(range(len(shape)), key=lambda i: -shape[i])
    if shape[order[1]] < MIN_DIM_SIZE_TO_FACTOR:
        return None
    return order[0], order[1]


def _rms(x):
    return np.sqrt(np.mean(np.square(x)))


def slot_names(name, shape, beta1):
    fd = factored_dims(shape)
    out = [name + "_slot_vr", name + "_slot_vc"] if fd is not None else [name + "_slot_v"]
    return out + ([name + "_slot_m"] if beta1 else [])


def init_slots(shapes, beta1):
    """name -> shape: the zero-initialised slots of every variable"""
    s = OrderedDict()
    for name, shape in shapes.items():
        fd = factored_dims(shape)
        if fd is not None:
            s[name + "_slot_vr"] = np.zeros(shape[fd[1]])
            s[name + "_slot_vc"] = np.zeros(shape[fd[0]])
        else:
            s[name + "_slot_v"] = np.zeros(shape)
        if beta1:
            s[name + "_slot_m"] = np.zeros(shape)
    return s


def apply_grad(name, w, g, slots, lr, decay=0.0, beta1=0.9, eps1=1e-30, eps2=1e-3):
    """one variable: returns the new w (float64); updates `slots` in place"""
    w = np.asarray(w, np.float64)
    g = np.asarray(g, np.float64)
    g2 = g * g + eps1
    scale = lr * max(_rms(w), eps2)
    fd = factored_dims(w.shape)
    if fd is not None:
        d0, d1 = fd
        vr = decay * slots[name + "_slot_vr"] + (1 - decay) * g2.mean(axis=d0)    # indexed along d1
        vc = decay * slots[name + "_slot_vc"] + (1 - decay) * g2.mean(axis=d1)    # indexed along d0
        slots[name + "_slot_vr"], slots[name + "_slot_vc"] = vr, vc
        shp_r, shp_c = [1] * w.ndim, [1] * w.ndim
        shp_r[d1], shp_c[d0] = w.shape[d1], w.shape[d0]
        x = g / np.sqrt((vr / vr.mean()).reshape(shp_r)) / np.sqrt(vc.reshape(shp_c))
    else:
        v = decay * slots[name + "_slot_v"] + (1 - decay) * g2
        slots[name + "_slot_v"] = v
        x = g / np.sqrt(v)
    x = x / max(1.0, _rms(x) / CLIPPING_THRESHOLD)
    u = scale * x
    if beta1:
        m = beta1 * slots[name + "_slot_m"] + (1 - beta1) * u
        slots[name + "_slot_m"] = m
        u = m
    return w - u


def apply_grads(params, grads, slots, lr, decay=0.0, beta1=0.9, eps1=1e-30, eps2=1e-3):
    """every variable (params / grads: name -> array); returns the new params (float64), updates `slots` in place"""
    return OrderedDict((n, apply_grad(n, params[n], grads[n], slots, lr, decay, beta1, eps1, eps2)) for n in params)


def train(params, tokens, cfg, hp, steps, start_step, slots=None):
    """`steps` reference train steps from global step `start_step`: gradients of the fp32 oracle at the current (float64) weights,
    clip_by_global_norm, the scheduled learning rate, then the float64 Adafactor update.  Returns (params, slots, losses)."""
    a = hyper_parameters(hp)
    P = OrderedDict((n, np.asarray(v, np.float64)) for n, v in params.items())
    if slots is None:
        slots = init_slots(OrderedDict((n, v.shape) for n, v in P.items()), a["beta1"])
    losses = []
    for i in range(steps):
        step = start_step + i
        loss, grads = do.loss_and_grads(OrderedDict((n, v.astype(np.float32)) for n, v in P.items()), tokens, cfg)
        losses.append(loss)
        clip = hp.get("gradient_clipping", 1.0)
        if clip is not None:
            grads, _ = do.clip_by_global_norm(grads, clip)
        lr = do.learning_rate(step, hp["lr"], hp["train_steps"], hp.get("warmup_steps", 3000), hp.get("lr_decay", "cosine"),
                              hp.get("lr_decay_end"))
        P = apply_grads(P, grads, slots, lr, **a)
    return P, slots, losses
