"""src/vae_tf/lowering.py alone (no torch, no library) against tests/golden/vae_lowering.json, which
tests/golden/make_vae_lowering_golden.py read off constructed DiscreteVAE models: the flat parameter layout, the derived weight
copies with their offsets, the tables of the two batched refresh launches and the column scratch, for

  vae_example, vae_coco  the shipped shapes (every down / res layer implicit);
  unaligned              16- and 8-channel layers: materialised arms, padded transposes (9 * 16 = 144 -> pitch 192), one-tap head;
  nonpow2                grids 24 -> 12 -> 6 with 64-aligned channels: implicit input gradients, materialised forward / weight gradient;
  stacked                space_to_depth by 2 in front (12 image channels padded to 16).

The byte sizes of ws / ws_cs / ws_pool need the library's workspace functions: tests/test_vae_lowering_gpu.py checks those.  The
second test writes every product's implicit-or-materialised predicate out literally, per layer kind."""
import importlib.util
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "vae_lowering.json")))


def _load():
    """the module by path: importing the package would import models.py, and with it torch and the library"""
    spec = importlib.util.spec_from_file_location("vae_lowering", os.path.join(ROOT, "dalle-mtf_amd", "src", "vae_tf", "lowering.py"))
    before = set(sys.modules)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert not {m.split(".")[0] for m in set(sys.modules) - before} & {"torch", "dalle_hip", "numpy"}
    return mod


low = _load()


def _graph(cfg):
    s = cfg.get("stack_factor", 1)
    c_st = 3 * s * s
    return low.build_graph(cfg["dimensions"] // s, low._ru(c_st, 8), c_st, [tuple(b) for b in cfg["convblocks"]],
                           cfg["convblocks"][-1][1], cfg["num_tokens"])


def test_the_five_configurations_are_there():
    assert sorted(GOLDEN) == ["nonpow2", "stacked", "unaligned", "vae_coco", "vae_example"]
    assert GOLDEN["unaligned"]["padded"] and GOLDEN["unaligned"]["config"]["batch_size"] == 2
    assert GOLDEN["stacked"]["config"]["stack_factor"] == 2


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_layouts_tables_and_column_scratch_equal_the_recorded_ones(name):
    G = GOLDEN[name]
    cfg = G["config"]
    n_hid, T = cfg["convblocks"][-1][1], cfg["num_tokens"]
    convs, n_enc, offset, shape, total = _graph(cfg)
    assert offset == G["offset"] and list(offset) == sorted(G["offset"], key=G["offset"].get)
    assert {k: list(v) for k, v in shape.items()} == G["shape"] and total == G["total"]
    plan, wc_off, numel = low.weight_copies(convs, n_hid, T)
    assert [[kind, nm, q, wc_off[(kind, nm, q)], rows, cols] for kind, nm, q, rows, cols in plan] == G["weight_copies"]
    assert numel == G["wcopies_numel"]
    R = low.refresh_tables(convs, offset, wc_off, n_hid, T)
    assert R["tr"] == G["tr"] and R["tiles"] == G["tiles"]
    assert (R["ga"] or None) == G["ga"] and R["blocks"] == G["blocks"]
    assert [list(p) for p in R["padded"]] == G["padded"]
    assert low.max_col(convs, cfg["batch_size"]) == G["col_numel"]


def _p2(v):
    return v > 0 and (v & (v - 1)) == 0


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_every_product_states_its_predicate(name):
    convs = _graph(GOLDEN[name]["config"])[0]
    kinds = set()
    for c in convs:
        kinds.add(c.kind)
        fwd, wg, dg = [t.implicit for t in c.fwd], c.wgrad.implicit, [t.implicit for t in c.dgrad or ()]
        if c.kind in ("down", "res"):
            ok = c.cin % 64 == 0 and _p2(c.Ho) and _p2(c.Wo)
            assert low.implicit_ok(c) == ok and fwd == [ok] and wg == ok and c.wgrad is c.fwd[0]
            assert dg == [c.cout % 64 == 0] * (4 if c.kind == "down" else 1)
        elif c.kind == "up":
            assert fwd == [c.cin % 64 == 0] * 4
            assert wg == (c.cout % 64 == 0 and _p2(c.H) and _p2(c.W)) and c.dgrad == (c.wgrad,)
        else:
            assert fwd == [False] and not wg and c.dgrad is None        # the head gathers nothing inside a GEMM ...
            assert c.fwd[0].direct == (c.cin % 64 == 0) and c.wgrad.direct     # ... and reads x as its own column where the pitch allows
        for t in c.products() + (c.wgrad,):
            assert t.K == len(t.taps) * t.C and t.Kp == (t.K if t.direct else (t.K + 63) // 64 * 64) and not (t.implicit and t.direct)
    assert kinds == {"down", "res", "up", "final"}
    reached = {(c.kind, t.implicit) for c in convs for t in c.products()}
    if name in ("vae_example", "vae_coco"):
        assert all(c.fwd[0].implicit for c in convs if c.kind == "res")
    if name == "unaligned":
        assert {("down", False), ("res", False), ("up", False), ("up", True)} <= reached
    if name == "nonpow2":
        assert any(c.kind == "up" and not c.wgrad.implicit and c.cout % 64 == 0 for c in convs)
