"""The fp32 step oracle tests/dalle_step_ref.py against oracle.dalle_oracle on the CPU: with every switch off, and with every switch
at its identity value, it is oracle.dalle_oracle.loss_and_grads bit for bit; every switch alone moves the result; all of them
together run.  One torch thread: with more, the gather's backward sums embedding/wte's gradient in an order that changes from run
to run (about 1e-7 absolute, in oracle.dalle_oracle.loss_and_grads as well)."""
import numpy as np
import pytest
import torch

import dalle_step_ref as sref
import dropout_ref as dref
from engine_case import inputs
from oracle import dalle_oracle as do
from src.dalle_mtf.masks import layer_masks
from src.dalle_mtf.rotary import rotary_table

WIDTH, HEADS, LAYERS, T, P, B = 128, 2, 2, 16, 64, 2
S = T + P


@pytest.fixture(scope="module")
def case():
    """(cfg, P0, tokens, the all-off result, {switch: a value that is not its identity}); single-threaded until the module is done"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    cfg, P0, tokens = inputs(WIDTH, HEADS, LAYERS, B, T=T, P=P)
    t = dref.threshold(0.25)
    on = dict(masks=layer_masks(["row", "conv:3"], LAYERS, T, P), table=rotary_table("axial", T, P, cfg.kv_dim), token_shift=True,
              dropout=dref.engine_masks({s: (dref.site_key(0, 0, 0, 0, s), t) for s in range(2 + 2 * LAYERS)}, B, S, WIDTH, LAYERS),
              activation="gelu", loss_weights=(1.0, 7.0))
    yield cfg, P0, tokens, sref.loss_and_grads(P0, tokens, cfg), on
    torch.set_num_threads(threads)


def _same_bits(a, b):
    (la, ga), (lb, gb) = a, b
    return la == lb and list(ga) == list(gb) and all(np.array_equal(ga[k].view(np.uint32), gb[k].view(np.uint32)) for k in ga)


def test_all_switches_off_is_the_oracle_bit_for_bit(case):
    cfg, P0, tokens, off, _ = case
    assert _same_bits(off, do.loss_and_grads(P0, tokens, cfg))
    assert _same_bits(off, sref.loss_and_grads(P0, tokens, cfg, masks=None, table=None, token_shift=False, dropout=None,
                                               activation="relu", loss_weights=None))


def test_identity_values_reproduce_off(case):
    cfg, P0, tokens, off, _ = case
    causal = [np.tril(np.ones((S, S), bool))] * LAYERS
    ones = {s: np.ones((S, WIDTH) if s == 1 else (B, S, WIDTH), np.float32) for s in range(2 + 2 * LAYERS)}
    assert _same_bits(off, sref.loss_and_grads(P0, tokens, cfg, masks=causal))
    assert _same_bits(off, sref.loss_and_grads(P0, tokens, cfg, dropout=ones))
    assert _same_bits(off, sref.loss_and_grads(P0, tokens, cfg, loss_weights=None))
    # a zero-angle table rotates by x * 1 - y * 0: every value is kept, the sign of a zero need not be
    table = np.zeros((S, cfg.kv_dim // 2, 2), np.float32)
    table[..., 0] = 1.0
    loss, g = sref.loss_and_grads(P0, tokens, cfg, table=table)
    assert loss == off[0]
    for k in g:
        assert np.array_equal(g[k], off[1][k]), k


@pytest.mark.parametrize("switch", ["masks", "table", "token_shift", "dropout", "activation", "loss_weights"])
def test_each_switch_alone_moves_the_result(case, switch):
    cfg, P0, tokens, off, on = case
    loss, g = sref.loss_and_grads(P0, tokens, cfg, **{switch: on[switch]})
    assert loss != off[0] or any(not np.array_equal(g[k], off[1][k]) for k in g)


def test_all_switches_on(case):
    cfg, P0, tokens, off, on = case
    loss, g = sref.loss_and_grads(P0, tokens, cfg, **on)
    assert np.isfinite(loss) and loss != off[0]
    assert list(g) == list(P0)
    for k in g:
        assert g[k].shape == P0[k].shape and np.isfinite(g[k]).all() and np.any(g[k] != 0), k
