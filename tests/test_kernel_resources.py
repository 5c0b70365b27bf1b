"""Compile-time properties of the gfx950 kernels that performance depends on and that a run cannot see failing (CPU only:
hipcc cross-compiles without a GPU): every kernel keeps its working set in registers -- NO scratch memory (a spilled value's
reload waits with vmcnt(0), i.e. for every LDS-DMA and store the wave has in flight: the dQ attention kernel ran 128 us per layer
with 19 spilled registers and 113 us without, profiles/r04_step_breakdown.txt) -- and the kernels designed for two blocks per CU fit
two waves per SIMD.  The numbers come from the compiler's own -Rpass-analysis=kernel-resource-usage remarks."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
CSRC = os.path.join(ROOT, "dalle-mtf_amd", "csrc")
FILES = ("gemm.hip", "attention.hip", "elementwise.hip", "vae.hip")


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def usage():
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("hipcc not found")
    from dalle_hip import build as b
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        procs = [(f, subprocess.Popen([hipcc] + b.FLAGS + ["-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                                      os.path.join(CSRC, f), "-o", os.path.join(tmp, f + ".o")], stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT, text=True)) for f in FILES]
        for f, p in procs:
            text, _ = p.communicate()
            assert p.returncode == 0, text[-2000:]
            for blk in re.split(r"remark: Function Name: ", text)[1:]:
                g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))   # noqa: E731
                out[blk.split()[0]] = dict(file=f, vgpr=g(" VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                           occupancy=g(r"Occupancy \[waves/SIMD\]"), sgpr_spill=g("SGPRs Spill"), vgpr_spill=g("VGPRs Spill"))
    return out


def test_no_kernel_uses_scratch(usage):
    assert len(usage) > 100, len(usage)     # every template instantiation of the four files reports
    bad = {k: v for k, v in usage.items() if v["scratch"] or v["vgpr_spill"]}
    assert not bad, bad
    # scalar registers spilled into VGPR lanes (v_writelane / v_readlane, no memory) are tolerated where they exist today: a few
    # instantiations of the persistent 256x256 NT kernel, whose eight buffer descriptors and tile bookkeeping exceed the SGPR file,
    # and [r06] the software-pipelined attention forward kernel (two buffer descriptors, eight LDS-DMA destinations, the item schedule
    # and the next item's prefetch state: 45 lanes, all read / written at item boundaries -- the two 32-MFMA step bodies contain no
    # v_readlane / v_writelane, checked on the disassembly)
    sg = {k: v["sgpr_spill"] for k, v in usage.items() if v["sgpr_spill"]}
    assert all("gemm_nt8p_kernel" in k or "attn_fwd2_kernel" in k for k in sg), sg
    assert all(n <= (48 if "attn_fwd2_kernel" in k else 28) for k, n in sg.items()), sg


def test_two_blocks_per_cu_kernels_fit_two_waves_per_simd(usage):
    """launch_bounds(256, 2) kernels: 256 registers (VGPR + AGPR) per lane at most, reported occupancy >= 2; the dK/dV attention
    kernel is the one deliberate one-wave-per-SIMD kernel (252 + 256 registers)"""
    two = [k for k in usage if re.search(r"gemm_nt8p_kernel|gemm_ntr_kernel|gemm_nt8_kernel|gemm_tn_kernel|gemm_tn_tail_kernel|gemm_tn_wide_sk_kernel|conv_wgrad_tn_kernel|"
                                          r"conv_gemm_nt_kernel|attn_fwd_kernel|attn_fwd2_kernel|attn_bwd_dq_kernel", k)]
    assert len(two) >= 30, two
    for k in two:
        u = usage[k]
        assert u["occupancy"] >= 2 and u["vgpr"] + u["agpr"] <= 256, (k, u)
    dkv = [k for k in usage if "attn_bwd_dkv_kernel" in k and "Lb0E" in k]   # the causal instances (MASKED = false)
    assert len(dkv) == 2      # [r06] the round-2 epilogue (A/B arm) and the whole-row one
    for k in dkv:
        assert usage[k]["occupancy"] == 1 and usage[k]["vgpr"] + usage[k]["agpr"] <= 512, (k, usage[k])
