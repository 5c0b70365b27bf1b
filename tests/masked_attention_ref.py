"""The reference's additive attention mask from a bool one (the reference applies attn_mask as the attention bias,
src/dalle_mtf/models.py:292-299); the masked fp32 step oracle is tests/dalle_step_ref.py."""
import numpy as np
import torch


def additive(mask_bool):
    """bool [S, S] (True = attend) -> the reference's additive mask (0 / -1e10)"""
    return torch.from_numpy(np.where(mask_bool, 0.0, -1e10).astype(np.float32))
