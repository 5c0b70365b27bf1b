"""Head dim 64 (n_embd / n_heads = 64), CPU side: the head-dim C ABI (declared, exported, bound; argument errors come back as a
status and a message before anything is launched -- the pointers below are never dereferenced) and the compile-time resources of
the four head-dim-64 attention kernels (no scratch, no spills, the occupancy they are built for)."""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
import dalle_hip as dh  # noqa: E402

HD_SYMBOLS = ("dmi_attention_fwd_hd", "dmi_attention_bwd_hd", "dmi_attention_decode_hd")
FAKE = ctypes.c_void_p(0x10000)
DMI_ERR_INVALID, DMI_ERR_UNSUPPORTED = -1, -3


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def _fwd(hd, ptr=FAKE, S=128):
    return dh.lib().dmi_attention_fwd_hd(ptr, ptr, ptr, 1, 1, S, hd, None)


def _bwd(hd, ptr=FAKE, S=128):
    return dh.lib().dmi_attention_bwd_hd(ptr, ptr, ptr, ptr, ptr, ptr, 1, 1, S, hd, None)


def _dec(hd, ptr=FAKE, S=128, pos=0):
    return dh.lib().dmi_attention_decode_hd(ptr, None, ptr, 1, 1, S, pos, None, hd, None)


def test_head_dim_entry_points_are_declared_exported_and_bound():
    L = dh.lib()
    declared = dh.declared_symbols()
    for name in HD_SYMBOLS:
        assert name in declared, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    assert len(L.dmi_attention_fwd_hd.argtypes) == 8
    assert len(L.dmi_attention_bwd_hd.argtypes) == 11
    assert len(L.dmi_attention_decode_hd.argtypes) == 10


@pytest.mark.parametrize("hd", [32, 96, 256, 0, -64])
def test_unsupported_head_dims_are_refused_naming_the_supported_ones(hd):
    for call, prefix in ((_fwd, "attention_fwd"), (_bwd, "attention_bwd"), (_dec, "attention_decode")):
        assert call(hd) == DMI_ERR_UNSUPPORTED, (call, hd)
        msg = _msg()
        assert msg.startswith(prefix) and "64" in msg and "128" in msg, msg
        with pytest.raises(dh.DalleHipError):
            dh._check(call(hd), prefix)


@pytest.mark.parametrize("hd", [64, 128])
def test_argument_checks_at_both_head_dims(hd):
    for call, prefix in ((_fwd, "attention_fwd"), (_bwd, "attention_bwd"), (_dec, "attention_decode")):
        assert call(hd, ptr=None) == DMI_ERR_INVALID, (call, hd)
        msg = _msg()
        assert msg.startswith(prefix) and "null" in msg, msg
    for call, prefix in ((_fwd, "attention_fwd"), (_bwd, "attention_bwd")):
        assert call(hd, S=12) == DMI_ERR_INVALID
        msg = _msg()
        assert msg.startswith(prefix) and "multiple of 8" in msg, msg
        assert call(hd, S=0) == DMI_ERR_INVALID
    assert _dec(hd, pos=128) == DMI_ERR_INVALID and "0 <= pos < S" in _msg()
    assert _dec(hd, pos=-1) == DMI_ERR_INVALID


def test_head_dim64_32bit_offset_bound_is_refused():
    """(S + 64) * 3 * H * 64 * 2 must stay below 2^31: S = 65536, H = 86 is just past it, H = 85 inside -- only the refusal is
    called here (the accepted shape would launch)."""
    L = dh.lib()
    assert (65536 + 64) * 3 * 86 * 64 * 2 >= 2 ** 31 > (65536 + 64) * 3 * 85 * 64 * 2
    for fn, n in ((L.dmi_attention_fwd_hd, 3), (L.dmi_attention_bwd_hd, 6)):
        assert fn(*([FAKE] * n), 1, 86, 65536, 64, None) == DMI_ERR_INVALID
        assert "32-bit buffer offsets" in _msg()


# waves per SIMD the kernels are built for (csrc/attention.hip A64_*_WAVES): the forward and the dQ kernel at 168 registers (four waves,
# 128 registers, spilled), the dK/dV kernel at 256 (it holds dK^T, dV^T, K and V fragments and the stats of 16 rows)
A64_OCCUPANCY = {"attn64_fwd_kernel": 3, "attn64_bwd_dq_kernel": 3, "attn64_bwd_dkv_kernel": 2}


def test_head_dim64_kernels_use_no_scratch_and_reach_their_occupancy():
    from dalle_hip import build as b
    hipcc = b._hipcc()     # the compiler build() uses
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([hipcc] + b.FLAGS + ["-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(ROOT, "dalle-mtf_amd", "csrc", "attention.hip"), "-o", os.path.join(tmp, "a.o")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    usage = {}
    for blk in re.split(r"remark: Function Name: ", p.stdout)[1:]:
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))   # noqa: E731
        usage[blk.split()[0]] = dict(vgpr=g(" VGPRs"), agpr=g("AGPRs"), scratch=g(r"ScratchSize \[bytes/lane\]"),
                                     occupancy=g(r"Occupancy \[waves/SIMD\]"), sgpr_spill=g("SGPRs Spill"), vgpr_spill=g("VGPRs Spill"))
    # the three tile kernels and the head-dim-64 instance of the decode template (HEAD_DIM = 64, as the symbol spells it)
    mine = {k: v for k, v in usage.items() if "attn64_" in k or "attn_decode_kernelILi64E" in k}
    assert len(mine) == 4, sorted(mine)
    for k, u in mine.items():
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (k, u)
    for name, occ in A64_OCCUPANCY.items():
        (k,) = [k for k in mine if name in k]
        assert mine[k]["occupancy"] == occ and mine[k]["vgpr"] + mine[k]["agpr"] <= 512 // occ, (k, mine[k])
