"""Weight EMA on the CPU: the ABI of dmi_ema_step and its refusals, the decay schedule, the config keys, the --weights argument,
and the kernel's compile-time resources."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import dalle_hip as dh  # noqa: E402
import ema_ref  # noqa: E402
from src.dalle_mtf.ema import ema_decay_at, one_minus_decay, resolve_ema, resolve_weights  # noqa: E402


def test_symbol_is_declared_exported_and_bound():
    assert "dmi_ema_step" in dh.declared_symbols()
    assert hasattr(ctypes.CDLL(dh.LIB_PATH), "dmi_ema_step")
    fn = dh.lib().dmi_ema_step
    assert fn.restype is ctypes.c_int
    assert list(fn.argtypes) == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p]
    assert callable(dh.ema_step)


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_abi_refusals():
    """every refusal comes before any launch: the fake pointers are never dereferenced"""
    L = dh.lib()
    a, b, c = 0x10000, 0x20000, 0x30000
    assert L.dmi_ema_step(None, b, c, 8, 0.5, None) == -1 and _msg().startswith("ema_step") and "null" in _msg()
    assert L.dmi_ema_step(a, None, c, 8, 0.5, None) == -1 and "null" in _msg()
    for n in (0, -4):
        assert L.dmi_ema_step(a, b, c, n, 0.5, None) == -1 and "n must be positive" in _msg(), n
    for args in ((a + 4, b, c), (a, b + 8, c), (a, b, c + 2), (a, b, c + 8)):
        assert L.dmi_ema_step(*args, 8, 0.5, None) == -1 and "16-byte aligned" in _msg(), args
    for omd in (float("nan"), -1e-3, 1.0 + 1e-6, float("inf"), -float("inf")):
        assert L.dmi_ema_step(a, b, c, 8, omd, None) == -1 and "one_minus_decay" in _msg(), omd
    with pytest.raises(dh.DalleHipError, match="one_minus_decay"):
        dh._check(L.dmi_ema_step(a, b, None, 8, 2.0, None), "ema_step")


def test_decay_schedule():
    d = 0.999
    first = next(t for t in range(10 ** 5) if (1.0 + t) / (10.0 + t) >= d)
    assert first == 8990                                     # (1 + t) / (10 + t) >= 0.999  <=>  t >= 8990
    for t in (0, 1, 9, 89, 10 ** 6, first - 1, first, first + 1):
        want = min(d, (1.0 + t) / (10.0 + t))
        assert ema_decay_at(d, t) == want == ema_ref.ema_decay_at(d, t), t
        assert one_minus_decay(d, t) == float(np.float32(1.0 - want)) == ema_ref.one_minus_decay(d, t)
    assert ema_decay_at(d, 0) == 0.1 and ema_decay_at(d, 89) == 90.0 / 99.0
    assert ema_decay_at(d, first - 1) < d and ema_decay_at(d, first) == d and ema_decay_at(d, 10 ** 6) == d
    assert 0.0 <= one_minus_decay(d, 10 ** 6) <= 1.0


def test_config_keys():
    assert resolve_ema(None) == (None, False) and resolve_ema({}) == (None, False)
    assert resolve_ema({"ema_decay": None}) == (None, False) and resolve_ema({"ema_decay": 0}) == (None, False)
    assert resolve_ema({"ema_decay": 0.999}) == (0.999, False)
    assert resolve_ema({"ema_decay": 0.99, "ema_eval": True}) == (0.99, True)
    assert resolve_ema({"ema_decay": 0.99, "ema_eval": False}) == (0.99, False)
    for bad in (1, 1.0, -0.1, float("nan"), float("inf"), "x", True, 1.5):
        with pytest.raises(ValueError, match="ema_decay"):
            resolve_ema({"ema_decay": bad})
    for params in ({"ema_eval": True}, {"ema_eval": True, "ema_decay": 0}, {"ema_eval": True, "ema_decay": None}):
        with pytest.raises(ValueError, match="ema_eval"):
            resolve_ema(params)
    with pytest.raises(ValueError, match="ema_eval"):
        resolve_ema({"ema_decay": 0.9, "ema_eval": "yes"})


def test_shipped_configs_leave_the_average_off():
    from src.utils import fetch_model_params
    for name in ("dalle_example", "dalle_coco"):
        p = fetch_model_params(name)
        assert resolve_ema({k: p[k] for k in ("ema_decay", "ema_eval")}) == (None, False)


def test_weights_choice():
    assert resolve_weights(None, True) == "ema" and resolve_weights(None, False) == "raw"
    assert resolve_weights("auto", True) == "ema" and resolve_weights("auto", False) == "raw"
    assert resolve_weights("raw", True) == "raw" and resolve_weights("raw", False) == "raw"
    assert resolve_weights("ema", True) == "ema"
    with pytest.raises(ValueError, match="no weight average"):
        resolve_weights("ema", False)
    with pytest.raises(ValueError):
        resolve_weights("mean", True)


def test_weights_argument_parses(capsys):
    from src.generate import build_parser
    base = ["--model", "dalle_example", "--from-eval", "1"]
    p = build_parser()
    assert p.parse_args(base).weights == "auto"
    for w in ("auto", "ema", "raw"):
        assert p.parse_args(base + ["--weights", w]).weights == w
    with pytest.raises(SystemExit) as e:
        p.parse_args(base + ["--weights", "mean"])
    assert e.value.code == 2 and "--weights" in capsys.readouterr().err


def test_reference_helpers():
    """the restatement itself: bf16 rounding to nearest even on the ties, and the three roundings of the update"""
    f = lambda bits: np.array([bits], np.uint32).view(np.float32)   # noqa: E731
    assert ema_ref.bf16_rne_bits(f(0x3F808000))[0] == 0x3F80       # tie, even below: down
    assert ema_ref.bf16_rne_bits(f(0x3F818000))[0] == 0x3F82       # tie, odd below: up
    assert ema_ref.bf16_rne_bits(f(0x3F808001))[0] == 0x3F81
    assert ema_ref.bf16_rne_bits(f(0x7F7FFFFF))[0] == 0x7F80       # rounds to +Inf
    assert math.isnan(float(ema_ref.bf16_to_f32(ema_ref.bf16_rne_bits(np.array([np.nan], np.float32)))[0]))
    e, p, omd = np.float32(1.0), np.float32(1e-8), np.float32(1e-3)
    want = np.float32(e - np.float32(np.float32(e - p) * omd))
    assert ema_ref.ema_step_ref([e], [p], omd)[0] == want
    assert ema_ref.ema_step_ref([e], [p], 0.0)[0] == e and ema_ref.ema_step_ref([e], [p], 1.0)[0] == np.float32(e - np.float32(e - p))


def test_kernel_keeps_its_working_set_in_registers():
    """no scratch, no spills (the compiler's kernel-resource-usage remarks, as tools/kres.py lists them)"""
    import shutil
    from dalle_hip import build as b
    if not (os.path.exists(b._hipcc()) or shutil.which(b._hipcc())):
        pytest.skip("hipcc not found")
    import kres
    u = {k: v for k, v in kres.usage("optim.hip").items() if "ema_kernel" in k}
    assert len(u) == 1, u
    v = next(iter(u.values()))
    assert v["scratch"] == 0 and v["vspill"] == 0 and v["sspill"] == 0, v
