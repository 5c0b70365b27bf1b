"""float64 restatement of mtf.gelu, the tanh form [MTF-RECALL: recalled from mesh-tensorflow 0.1.18, not checked against its
source], and its derivative; the fp32 step oracle (tests/dalle_step_ref.py, activation="gelu") puts it in the feed-forward.
  gelu(x)  = 0.5 x (1 + tanh(u)),  u = sqrt(2/pi) (x + 0.044715 x^3)
  gelu'(x) = 0.5 (1 + tanh(u)) + 0.5 x (1 - tanh(u)^2) u',  u' = sqrt(2/pi) (1 + 3 * 0.044715 x^2)"""
import math

import numpy as np
import torch

K0 = math.sqrt(2.0 / math.pi)
C3 = 0.044715


def gelu(x):
    """numpy or torch, in the input's precision (pass float64)"""
    tanh = torch.tanh if isinstance(x, torch.Tensor) else np.tanh
    return 0.5 * x * (1.0 + tanh(K0 * (x + C3 * x ** 3)))


def gelu_grad(x):
    tanh = torch.tanh if isinstance(x, torch.Tensor) else np.tanh
    t = tanh(K0 * (x + C3 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * K0 * (1.0 + 3.0 * C3 * x * x)
