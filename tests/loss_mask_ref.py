"""float64 restatement of the padded-caption loss mask (DESIGN.md §4 "Loss: padded caption positions"), independent of the
product's src/dalle_mtf/loss_mask.py.  Position p predicts token p + 1: rows p <= T - 2 of a sequence are text rows, rows p >= T - 1
image rows.  A text row whose label is the padding id is ignored; image rows never are.
  no weights:  loss = sum keep NLL / (n_t + n_i)
  (wt, wi):    loss = (wt L_t + wi L_i) / (wt + wi),  L_t = sum_text keep NLL / max(n_t, 1),  L_i = mean_image NLL"""
import numpy as np
import torch


def keep_ref(labels, split, pad):
    """labels int [B, S] -> (keep bool [B, S], n_t, n_i); text rows are the columns p < split (= T - 1)"""
    labels = np.asarray(labels)
    B, S = labels.shape
    keep = np.ones((B, S), bool)
    for b in range(B):
        for p in range(split):
            keep[b, p] = labels[b, p] != pad
    return keep, int(keep[:, :split].sum()), B * (S - split)


def row_weights_ref(labels, split, pad, weights=None):
    """float64 [B, S]: c[b, p] with loss = sum c NLL; weights = (wt, wi) or None (the no-weights formula)"""
    keep, n_t, n_i = keep_ref(labels, split, pad)
    c = np.zeros(keep.shape, np.float64)
    for (b, p), k in np.ndenumerate(keep):
        if weights is None:
            c[b, p] = float(k) / (n_t + n_i) if n_t + n_i else 0.0
        elif p < split:
            c[b, p] = float(k) * weights[0] / ((weights[0] + weights[1]) * max(n_t, 1))
        else:
            c[b, p] = weights[1] / ((weights[0] + weights[1]) * n_i)
    return c


def out4_ref(rows, labels, split, pad, weights, scale):
    """float64 restatement of dmi_loss_reduce_masked: rows, labels [B, S] -> (scale * sum c rows, L_t, L_i, n_t / text rows);
    a mean over no rows is 0"""
    rows = np.asarray(rows, np.float64)
    keep, n_t, n_i = keep_ref(labels, split, pad)
    c = row_weights_ref(labels, split, pad, weights)
    text = rows[:, :split][keep[:, :split]]
    n_text = rows.shape[0] * split
    return np.array([scale * (c * rows).sum(), text.sum() / n_t if n_t else 0.0, rows[:, split:].mean() if n_i else 0.0,
                     n_t / n_text if n_text else 0.0])


def masked_loss_ref(loss_batch, labels, T, pad, weights=None):
    """loss_batch [B, S] (numpy -> float64; a torch tensor keeps its dtype and autograd), labels int [B, S] ->
    (loss, L_t, L_i, n_t / (B (T - 1)))"""
    keep, n_t, n_i = keep_ref(labels, T - 1, pad)
    if isinstance(loss_batch, torch.Tensor):
        k = torch.as_tensor(keep[:, :T - 1], dtype=loss_batch.dtype)
    else:
        loss_batch = np.asarray(loss_batch, np.float64)
        k = keep[:, :T - 1].astype(np.float64)
    st = (loss_batch[:, :T - 1] * k).sum()
    si = loss_batch[:, T - 1:].sum()
    lt, li = st / max(n_t, 1), si / n_i
    loss = (st + si) / (n_t + n_i) if weights is None else (weights[0] * lt + weights[1] * li) / (weights[0] + weights[1])
    return loss, lt, li, n_t / (keep.shape[0] * (T - 1))
