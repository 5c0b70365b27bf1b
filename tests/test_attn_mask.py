"""Attention masks on the CPU: the pattern library against hand-written masks, the plan builder against a numpy classification,
refusals, the ABI, and the resources of the masked kernels (no scratch, no spills, the occupancy they are built for)."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))

import dalle_hip as dh  # noqa: E402
from src.dalle_mtf.masks import check_mask, layer_masks, pattern_mask, to_bool_mask  # noqa: E402

T, W = 4, 4
P = W * W


def _hand(rule):
    S = T + P
    m = np.tril(np.ones((S, S), dtype=bool))
    for i in range(P):
        for j in range(P):
            if j <= i:
                m[T + i, T + j] = rule(i // W, i % W, j // W, j % W) or i == j
    return m


def test_patterns_against_hand_written_masks():
    assert (pattern_mask("causal", T, P) == np.tril(np.ones((T + P,) * 2, dtype=bool))).all()
    assert (pattern_mask("row", T, P) == _hand(lambda r, c, r2, c2: r == r2)).all()
    assert (pattern_mask("column", T, P) == _hand(lambda r, c, r2, c2: c == c2)).all()
    assert (pattern_mask("conv:3", T, P) == _hand(lambda r, c, r2, c2: r - r2 <= 2 and abs(c2 - c) <= 1)).all()
    assert (pattern_mask("local:5", T, P) == _hand(lambda r, c, r2, c2: (r * W + c) - (r2 * W + c2) <= 5)).all()


@pytest.mark.parametrize("name", ["causal", "local:3", "row", "column", "conv:3", "conv:5"])
def test_patterns_are_causal_nonempty_and_see_all_text(name):
    m = pattern_mask(name, T, P)
    check_mask(m, T + P)
    assert m[T:, :T].all()


def test_pattern_refusals():
    for bad in ("diag", "local:x", "local:-1", "conv:2", "conv:", "row:1"):
        with pytest.raises(ValueError):
            pattern_mask(bad, T, P)
    with pytest.raises(ValueError, match="perfect square"):
        pattern_mask("row", T, 15)


def test_mask_spec_refusals():
    S = T + P
    with pytest.raises(ValueError, match="not causal"):
        to_bool_mask(np.ones((S, S), dtype=bool), T, P)
    empty = np.tril(np.ones((S, S), dtype=bool))
    empty[5] = False
    with pytest.raises(ValueError, match="no key"):
        to_bool_mask(empty, T, P)
    with pytest.raises(ValueError, match="shape"):
        to_bool_mask(np.tril(np.ones((S - 1, S - 1), dtype=bool)), T, P)
    add = np.where(np.tril(np.ones((S, S), dtype=bool)), 0.0, -1e10)
    assert (to_bool_mask(add, T, P) == np.tril(np.ones((S, S), dtype=bool))).all()
    with pytest.raises(ValueError, match="additive"):
        to_bool_mask(np.where(add == 0, 0.0, -5.0), T, P)
    with pytest.raises(ValueError, match="n_layers"):
        layer_masks(["row", "column"], 3, T, P)
    assert len(layer_masks(["row", "column", "causal"], 3, T, P)) == 3


# ---- the plan builder (host only) against a numpy classification
def _plan(m):
    return dh.AttnMaskPlan(m, device=None).host


HDR = dh.PLAN_HDR


def _sections(h):
    NB = h[HDR["NB"]]
    fptr = h[h[HDR["FPTR"]]:h[HDR["FPTR"]] + NB + 1]
    flist = h[h[HDR["FLIST"]]:h[HDR["FLIST"]] + fptr[-1]]
    kptr = h[h[HDR["KPTR"]]:h[HDR["KPTR"]] + NB + 1]
    klist = h[h[HDR["KLIST"]]:h[HDR["KLIST"]] + kptr[-1]]
    return NB, fptr, flist, kptr, klist


def _block_mask(S, seed):
    rng = np.random.default_rng(seed)
    nb = (S + 31) // 32
    m = np.kron(rng.random((nb, nb)) < 0.4, np.ones((32, 32), dtype=bool))[:S, :S]
    m |= rng.random((S, S)) < 0.02
    m &= np.tril(np.ones((S, S), dtype=bool))
    m[np.arange(S), np.arange(S)] = True
    return m


@pytest.mark.parametrize("S,seed", [(256, 0), (272, 1), (520, 2), (1280, 3)])
def test_plan_classifies_tiles(S, seed):
    m = _block_mask(S, seed)
    h = _plan(m)
    assert h[0] == dh.PLAN_MAGIC and h[HDR["S"]] == S and h[HDR["CAUSAL"]] == 0
    NB, fptr, flist, kptr, klist = _sections(h)
    Wd = (S + 31) // 32
    pad = np.zeros((NB * 128, NB * 128), dtype=bool)
    pad[:S, :S] = m
    for qb in range(NB):
        want = []
        for j in range((S + 63) // 64):
            cls = 0
            for w in range(4):
                r0 = qb * 128 + 32 * w
                if r0 >= S:
                    continue
                t = pad[r0:min(r0 + 32, S), 64 * j:64 * j + 64]
                c = 0 if not t.any() else (1 if t.all() and 64 * j + 64 <= S else 2)
                cls |= c << (2 * w)
            if cls:
                want.append(j | (cls << 16))
        assert list(flist[fptr[qb]:fptr[qb + 1]]) == want, qb
    for kb in range(NB):
        want = []
        for qi in range(Wd):
            t = m[32 * qi:32 * qi + 32, 128 * kb:128 * kb + 128]
            if t.any():
                want.append(qi | ((0 if t.all() else 1) << 16))
        assert list(klist[kptr[kb]:kptr[kb + 1]]) == want, kb
    for sec, ptr in ((h[HDR["FORDER"]], fptr), (h[HDR["KORDER"]], kptr)):   # work orders: a permutation, heaviest first
        order = h[sec:sec + NB]
        assert sorted(order) == list(range(NB))
        counts = [ptr[i + 1] - ptr[i] for i in order]
        assert counts == sorted(counts, reverse=True)
    rows = h[h[HDR["ROWBITS"]]:h[HDR["ROWBITS"]] + S * Wd].view(np.uint32).reshape(S, Wd)
    cols = h[h[HDR["COLBITS"]]:h[HDR["COLBITS"]] + S * Wd].view(np.uint32).reshape(S, Wd)
    bits = np.unpackbits(rows.view(np.uint8).reshape(S, Wd, 4), axis=2, bitorder="little").reshape(S, Wd * 32)[:, :S]
    assert (bits.astype(bool) == m).all()
    cbits = np.unpackbits(cols.view(np.uint8).reshape(S, Wd, 4), axis=2, bitorder="little").reshape(S, Wd * 32)[:, :S]
    assert (cbits.astype(bool) == m.T).all()


def test_causal_plan_is_flagged_and_row_pattern_removes_work():
    S = 1280
    assert _plan(np.tril(np.ones((S, S), dtype=bool)))[HDR["CAUSAL"]] == 1
    p = dh.AttnMaskPlan(pattern_mask("row", 256, 1024), device=None)
    assert not p.causal and p.live_fraction() < 0.6


def test_plan_builder_refusals():
    S = 64
    bad = np.ones((S, S), dtype=np.uint8)
    assert dh.attn_mask_plan_bytes(bad, S) == -1
    assert "not causal" in dh.lib().dmi_last_error_string().decode()
    e = np.tril(np.ones((S, S), dtype=np.uint8))
    e[3] = 0
    assert dh.attn_mask_plan_bytes(e, S) == -1
    assert "no key" in dh.lib().dmi_last_error_string().decode()
    assert dh.attn_mask_plan_bytes(np.tril(np.ones((60, 60), dtype=np.uint8)), 60) == -1
    assert dh.lib().dmi_attn_mask_plan(None, 64, None, 0) == -1


FAKE = 0x1000


def test_masked_abi_refusals():
    L = dh.lib()
    good = dh.AttnMaskPlan(pattern_mask("row", 16, 256), device=None).host
    causal = dh.AttnMaskPlan(np.tril(np.ones((272, 272), dtype=bool)), device=None).host
    msg = lambda: L.dmi_last_error_string().decode()  # noqa: E731
    assert L.dmi_attention_fwd_masked(FAKE, FAKE, FAKE, None, good.ctypes.data, 1, 1, 272, 128, None) == -1
    assert L.dmi_attention_fwd_masked(FAKE, FAKE, FAKE, FAKE, good.ctypes.data, 1, 1, 264, 128, None) == -1
    assert "built for S=272" in msg()
    assert L.dmi_attention_fwd_masked(FAKE, FAKE, FAKE, FAKE, good.ctypes.data, 1, 1, 272, 64, None) == -3
    assert "head dim 128" in msg()
    assert L.dmi_attention_bwd_masked(FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, good.ctypes.data, 1, 1, 272, 64, None) == -3
    assert L.dmi_attention_decode_masked(FAKE, None, FAKE, FAKE, good.ctypes.data, 1, 1, 272, 0, None, 64, None) == -3
    assert L.dmi_attention_bwd_masked(FAKE, None, FAKE, FAKE, FAKE, FAKE, FAKE, good.ctypes.data, 1, 1, 272, 128, None) == -1
    junk = np.zeros(64, dtype=np.int32)
    assert L.dmi_attention_fwd_masked(FAKE, FAKE, FAKE, FAKE, junk.ctypes.data, 1, 1, 272, 128, None) == -1
    assert "not a mask plan" in msg()
    # a causal plan routes to the causal entry points, whose own head-dim check applies (64 or 128)
    assert L.dmi_attention_fwd_masked(FAKE, FAKE, FAKE, FAKE, causal.ctypes.data, 1, 1, 272, 96, None) == -3
    assert dh.get_option("attn_mask_force") == 0


def test_mask_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "dalle_hip.h")).read()
    for name in ("dmi_attn_mask_plan", "dmi_attention_fwd_masked", "dmi_attention_bwd_masked", "dmi_attention_decode_masked"):
        assert re.search(r"\b" + name + r"\(", hdr), name
        fn = getattr(dh.lib(), name)
        assert fn.argtypes is not None, name
    try:
        dh.set_option("attn_mask_force", 1)
        assert dh.get_option("attn_mask_force") == 1
    finally:
        dh.set_option("attn_mask_force", 0)
    assert dh.get_option("attn_mask_force") == 0


# the masked instances (MASKED = true, as the symbol spells it) of the forward, dQ, dK/dV and decode templates
MASKED = {"attn_fwd_kernelILb1E": 2, "attn_bwd_dq_kernelILi1ELb1E": 2, "attn_bwd_dkv_kernelILi1ELb1E": 1, "attn_decode_kernelILi128ELb1E": 4}


def test_masked_kernels_use_no_scratch_and_reach_their_occupancy():
    from dalle_hip import build as b
    hipcc = b._hipcc()
    with tempfile.TemporaryDirectory() as td:
        p = subprocess.run([hipcc] + b.FLAGS + ["-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(ROOT, "dalle-mtf_amd", "csrc", "attention.hip"), "-o", os.path.join(td, "a.o")],
                           capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    usage = {}
    for blk in p.stderr.split("Function Name: ")[1:]:
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))  # noqa: E731
        usage[blk.split()[0]] = dict(vgpr=g(" VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                     occupancy=g(r"Occupancy \[waves/SIMD\]"), sgpr_spill=g("SGPRs Spill"), vgpr_spill=g("VGPRs Spill"))
    for k, occ in MASKED.items():
        (u,) = [v for n, v in usage.items() if k in n]
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (k, u)
        assert u["occupancy"] >= occ, (k, u)


def test_plan_header_names_match_the_kernel_enum():
    src = open(os.path.join(ROOT, "dalle-mtf_amd", "csrc", "attn_plan.h")).read()
    enum = re.search(r"enum \{\s*(AMP_S = 1[^}]*)\}", src).group(1)
    names = [n.strip().split("=")[0].strip() for n in enum.split(",") if n.strip()]
    assert {n[4:]: i + 1 for i, n in enumerate(names)} == dh.PLAN_HDR
    assert "#define AMP_MAGIC 0x504d4144" in src and dh.PLAN_MAGIC == 0x504D4144


def test_dalle_refuses_bad_masks_before_touching_the_gpu():
    from src.dalle_mtf.models import DALLE
    kw = dict(n_embd=256, text_vocab_size=64, image_vocab_size=32, text_seq_len=16, image_seq_len=256, n_layers=3, n_heads=2,
              batch_size=1)
    S = 272
    with pytest.raises(ValueError, match="not causal"):
        DALLE(attn_mask=np.ones((S, S), dtype=bool), **kw)
    with pytest.raises(ValueError, match="n_layers"):
        DALLE(attn_mask=["row", "column"], **kw)
    with pytest.raises(ValueError, match="unknown attention pattern"):
        DALLE(attn_mask="diagonal", **kw)
    with pytest.raises(ValueError, match="additive"):
        DALLE(attn_mask=np.where(np.tril(np.ones((S, S))), 0.0, -1.0).astype(np.float32), **kw)
    with pytest.raises(ValueError, match="shape"):
        DALLE(attn_mask=np.tril(np.ones((S - 8, S - 8), dtype=bool)), **kw)
    with pytest.raises(ValueError, match="attention_pattern"):
        DALLE(params={"attention_pattern": 3}, **kw)
    with pytest.raises(ValueError, match="n_layers"):
        DALLE(params={"attention_pattern": ["row", "row"]}, **kw)
    with pytest.raises(ValueError, match="perfect square"):
        DALLE(params={"attention_pattern": "row"}, **dict(kw, image_seq_len=240))
