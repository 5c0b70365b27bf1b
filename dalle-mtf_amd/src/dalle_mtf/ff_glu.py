"""Gated feed-forward: the config key "ff_glu" (DESIGN.md §4 "Gated feed-forward"; a project extension, the reference has none).

With the key on, the block's MLP is a gated linear unit in dalle-pytorch's chunk order (value first, gate second):

    a = xn2 . W1 + b1                       W1: [d, 8d], b1: [8d]   (the reference's names, layer_i/mlp/mlp_linear_1/{kernel,bias})
    h = a[:, :4d] * act(a[:, 4d:])          act = the config key "activation_fn": "gelu" -> GEGLU, "relu" (the default) -> ReGLU
    y = h . W2 + b2                         W2: [4d, d], as without the key

The hidden width stays 4d, so a layer gains 4 d^2 + 4d parameters.  "gelu" is the project's tanh form (dalle_mtf.activations);
dalle-pytorch's GEGLU uses the erf form.  It is part of the model (training, evaluation and every sampler).  The key absent, None
or False: off -- the same buffers and launches as before.  Pure host code: nothing here touches a device."""

KEY = "ff_glu"


def resolve_ff_glu(params):
    """the config key as a bool: absent, None and False are off, True is on; anything else raises ValueError naming the key"""
    on = (params or {}).get(KEY)
    if on is None or on is False:
        return False
    if on is not True:
        raise ValueError(f"config key {KEY}: expected true, or null / false for off (got {on!r})")
    return True


def ffn1_width(n_embd, glu):
    """the output width of mlp_linear_1: [value | gate] = 8d gated, 4d plain"""
    return (8 if glu else 4) * int(n_embd)
