"""float64 restatement of the text/image loss weights (DESIGN.md §4 "Loss weights"), independent of the product's builder.
Position p predicts token p + 1 (reference src/dalle_mtf/models.py:407-410): positions p <= T - 2 predict text, p >= T - 1 predict
the P image tokens and EOS.
  loss = (wt * mean_text(NLL) + wi * mean_image(NLL)) / (wt + wi),  both means over the batch"""
import numpy as np
import torch


def position_weights_ref(T, P, wt, wi):
    """float64 [T + P]: w[p] = wt / ((wt + wi)(T - 1)) for text positions, wi / ((wt + wi)(P + 1)) for image positions"""
    w = np.zeros(T + P, np.float64)
    for p in range(T + P):
        w[p] = wt / ((wt + wi) * (T - 1)) if p <= T - 2 else wi / ((wt + wi) * (P + 1))
    return w


def weighted_loss_ref(loss_batch, T, wt, wi):
    """loss_batch [B, S] (numpy -> float64; a torch tensor keeps its dtype and autograd) -> (loss, mean_text, mean_image)"""
    if not isinstance(loss_batch, torch.Tensor):
        loss_batch = np.asarray(loss_batch, np.float64)
    mt, mi = loss_batch[:, :T - 1].mean(), loss_batch[:, T - 1:].mean()
    return (wt * mt + wi * mi) / (wt + wi), mt, mi


def loss_reduce_ref(rows, w, split, scale):
    """float64 restatement of dmi_loss_reduce: rows [n], w [period] -> (scale * sum w[m % period] rows[m], mean over m % period < split,
    mean over the rest)"""
    rows, w = np.asarray(rows, np.float64), np.asarray(w, np.float64)
    pos = np.arange(rows.size) % w.size
    return np.array([scale * (w[pos] * rows).sum(), rows[pos < split].mean(), rows[pos >= split].mean()])
