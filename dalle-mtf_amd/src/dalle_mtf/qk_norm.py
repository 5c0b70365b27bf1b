"""QK normalisation: the config key "qk_norm" (DESIGN.md §4 "QK norm"; a project extension, the reference has none).

With the key on, every head's query and key vectors of every layer are RMS-normalised over the head's head_dim channels behind the QKV
projection -- and before the rotation when "rotary_emb" is on -- with learned gains shared by the heads of a layer:

    r(x) = rsqrt(mean_j(x_j^2) + EPS)       the mean over the head's channels, in fp32
    q'   = q * r(q) * g_q * head_dim^(-1/2)  g_q: layer_i/attn/q_norm/g, [head_dim], initialised to 1
    k'   = k * r(k) * g_k                    g_k: layer_i/attn/k_norm/g, [head_dim], initialised to 1

The constant head_dim^(-1/2) stands in for the scale that attn/q's initialiser carries without the key and that the normalisation
removes; the attention kernels keep their unscaled-logit contract.  v is not touched.  EPS is fixed: there is no key for it.  It is
part of the model (training, evaluation and every sampler).  The key absent, None or False: off -- the same variables, buffers and
launches as before.  Pure host code: nothing here touches a device."""

KEY = "qk_norm"
EPS = 1e-6
GAIN_NAMES = ("attn/q_norm/g", "attn/k_norm/g")     # behind "layer_i/"; both [head_dim]


def resolve_qk_norm(params):
    """the config key as a bool: absent, None and False are off, True is on; anything else raises ValueError naming the key"""
    on = (params or {}).get(KEY)
    if on is None or on is False:
        return False
    if on is not True:
        raise ValueError(f"config key {KEY}: expected true, or null / false for off (got {on!r})")
    return True


def q_scale(head_dim):
    """the constant factor of the normalised queries, head_dim^(-1/2); the keys' is 1"""
    return float(head_dim) ** -0.5
