"""The FFN activation of DALLE(activation_fn=...) and the "activation_fn" config key (DESIGN.md §4 "GELU").

The reference applies `activation_fn` to the MLP's hidden layer only (src/dalle_mtf/models.py:317-324, default mtf.relu).  The
kernels implement two of them, named by string:
  relu   max(x, 0)                                                      (the reference's default)
  gelu   0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))                 (mtf.gelu, the tanh form [MTF-RECALL])
[MTF-RECALL]: the tanh form of mtf.gelu is recalled from mesh-tensorflow 0.1.18, which was not available to check against."""

ACTIVATIONS = ("relu", "gelu")
DEFAULT = "relu"


def check_activation(name):
    """a supported activation name, unchanged; anything else raises NotImplementedError"""
    if not isinstance(name, str) or name not in ACTIVATIONS:
        what = f"callable {getattr(name, '__name__', type(name).__name__)}" if callable(name) else repr(name)
        raise NotImplementedError(f"activation_fn {what}: the kernels implement {' and '.join(map(repr, ACTIVATIONS))} "
                                  "(pass the name as a string)")
    return name


def resolve_activation(activation_fn=None, params=None):
    """DALLE's activation: the argument if given, else the config key "activation_fn", else "relu"."""
    name = activation_fn
    if name is None and params:
        name = params.get("activation_fn")
    return check_activation(DEFAULT if name is None else name)
