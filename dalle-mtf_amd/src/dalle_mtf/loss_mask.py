"""Padded caption positions in the loss: the config key "loss_ignore_padding" (DESIGN.md §4 "Loss: padded caption positions").

Captions are right-padded to text_seq_len with the padding id, and the reference's loss (src/dalle_mtf/models.py:348-359) trains
on and reports every one of those labels.  With the key on, a text position whose LABEL is the padding id is ignored.  Position p
predicts token p + 1 (models.py:407-410): the rows p <= T - 2 of a sequence are text rows, the P + 1 rows p >= T - 1 image rows
(their labels are image tokens and EOS, never the padding id, and they are never ignored).  Per forward call of B sequences:
    keep[b, p] = 1 on image rows, (label[b, p] != pad) on text rows;  n_t = sum_text keep,  n_i = B (P + 1)
    no loss weights:  loss = sum keep NLL / (n_t + n_i)                                  c = keep / (n_t + n_i)
    weights (wt, wi): loss = (wt L_t + wi L_i) / (wt + wi),  L_t = sum_text keep NLL / max(n_t, 1),  L_i = mean_image NLL
                      c = keep wt / ((wt + wi) max(n_t, 1)) on text rows,  wi / ((wt + wi) n_i) on image rows
so that loss = sum c NLL in both; with n_t = 0, L_t = 0 and nothing is renormalised.  Every micro-batch of every rank is normalised
by its own counts and the step averages them with equal weight: the mean of masked means, not the global masked mean when the
counts differ.  A training setting like the loss weights, kept beside dalle_mtf.options: checkpoints and generate.json do not
record it, the sampler never sees it.  Pure host code."""
import numpy as np

KEY = "loss_ignore_padding"


def resolve_loss_ignore_padding(params, text_seq_len, text_vocab_size):
    """(on, pad_id) from the config key: unset, None and False are off -> (False, None); only a bool is accepted.  On: pad_id =
    params["padding_id"] when set, else text_vocab_size - 1 (the rule of src/input_fns.py and of the sampler's null caption); it must
    lie in [0, text_vocab_size), and text_seq_len must be >= 2.  Anything else raises ValueError naming the key."""
    v = (params or {}).get(KEY)
    if v is None or v is False:
        return False, None
    if v is not True:
        raise ValueError(f"config key {KEY}: expected true or false (got {v!r})")
    if text_seq_len < 2:
        raise ValueError(f"config key {KEY}: text_seq_len must be >= 2 (got {text_seq_len}): with one caption token no position "
                         "predicts text")
    pad = params.get("padding_id")
    if pad is None:
        pad = text_vocab_size - 1
    if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or not (0 <= pad < text_vocab_size):
        raise ValueError(f"config key {KEY}: padding_id must be an integer in [0, {text_vocab_size}) (got {pad!r})")
    return True, int(pad)


def mask_coefficients(loss_weights):
    """(ct, ci, plain): ct = wt / (wt + wi) and ci = wi / (wt + wi) in float64, what dmi_loss_mask forms its numerators from;
    loss_weights None: the no-weights formula (plain)"""
    if loss_weights is None:
        return 1.0, 1.0, True
    wt, wi = (float(w) for w in loss_weights)
    return wt / (wt + wi), wi / (wt + wi), False


def row_weights(labels, text_seq_len, pad_id, loss_weights=None):
    """float64 restatement of dmi_loss_mask: labels int [B, S] (labels[b, p] = the token position p predicts) ->
    (c [B, S], n_t, n_i) with loss = sum c NLL (module docstring)"""
    labels = np.asarray(labels)
    B, S = labels.shape
    T = int(text_seq_len)
    keep = np.ones((B, S), np.float64)
    keep[:, :T - 1] = labels[:, :T - 1] != pad_id
    n_t, n_i = int(keep[:, :T - 1].sum()), B * (S - T + 1)
    ct, ci, plain = mask_coefficients(loss_weights)
    if plain:
        return keep / max(n_t + n_i, 1), n_t, n_i
    c = np.empty((B, S), np.float64)
    c[:, :T - 1] = keep[:, :T - 1] * ct / max(n_t, 1)
    c[:, T - 1:] = ci / n_i
    return c, n_t, n_i


def log_line(pad_id, loss_weights):
    """the line the model function logs when the key is on"""
    return ("loss ignores padded caption positions: text labels equal to padding id %d carry no loss and no gradient; "
            "%s, every micro-batch normalised by its own counts" %
            (pad_id, "loss = sum over kept positions / their number" if loss_weights is None else
             "loss_text = mean over the kept caption labels"))
