"""Adafactor (src/optimizers.py:91-97), CPU side: get_optimizer's selection and argument mapping, the factoring decision for every
reference variable of the shipped model sizes, the float64 restatement against the reference-over-shim fixture
(tests/golden/ref_callsite_adafactor.npz), the C ABI's argument checks (nothing is launched) and the compile-time resources of
the six kernels of csrc/optim.hip."""
import ctypes
import importlib.util
import json
import os
import re
import subprocess
import sys
import tempfile
from collections import OrderedDict

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, HERE)
import adafactor_ref as ar  # noqa: E402
import dalle_hip as dh  # noqa: E402
from oracle import dalle_oracle as do  # noqa: E402
from src import optimizers  # noqa: E402
from src.dalle_mtf.engine import ParamLayout, adafactor_factored_dims  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "ref_callsite_adafactor.npz")
_spec = importlib.util.spec_from_file_location("make_adafactor_golden", os.path.join(HERE, "golden", "make_adafactor_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)


class _Engine:
    """what get_optimizer touches of DalleEngine"""

    def __init__(self):
        self.hp, self.chosen = {}, None

    def set_optimizer(self, name):
        self.chosen = name

    def learning_rate(self, step=None):
        return 0.0

    def optimizer_step(self):
        return self.chosen


@pytest.mark.parametrize("name", ["adafactor", "Adafactor", "ADAFACTOR", "adam", "Adam", None])
def test_get_optimizer_accepts_adam_and_adafactor(name):
    eng = _Engine()
    params = {"lr": 1e-3, "train_steps": 10}
    if name is not None:
        params["optimizer"] = name
    _, update = optimizers.get_optimizer(eng, params)
    assert update() == (name or "adam").lower()


@pytest.mark.parametrize("name", ["sgd", "adamw", "lamb", "adafactor2"])
def test_get_optimizer_refuses_other_names(name):
    with pytest.raises(ValueError, match=f"^{name} not recognized$"):
        optimizers.get_optimizer(_Engine(), {"optimizer": name, "lr": 1e-3, "train_steps": 10})


def test_hyper_parameter_mapping():
    """weight_decay is Adafactor's second-moment decay rate; beta_1, epsilon_1, epsilon_2 keep the reference's defaults"""
    assert ar.hyper_parameters({}) == dict(decay=0.0, beta1=0.9, eps1=1e-30, eps2=1e-3)
    assert ar.hyper_parameters({"weight_decay": 0.01, "beta_1": 0.0, "epsilon_1": 1e-20, "epsilon_2": 1e-2}) == \
        dict(decay=0.01, beta1=0.0, eps1=1e-20, eps2=1e-2)
    eng = _Engine()
    optimizers.get_optimizer(eng, {"optimizer": "adafactor", "lr": 1e-3, "train_steps": 10, "weight_decay": 0.01, "beta_1": 0.0,
                                   "epsilon_1": 1e-20, "epsilon_2": 1e-2})
    assert eng.hp["weight_decay"] == 0.01 and eng.hp["beta_1"] == 0.0
    assert eng.hp["epsilon_1"] == 1e-20 and eng.hp["epsilon_2"] == 1e-2 and eng.hp["gradient_clipping"] == 1.0


def _reference_shapes(d, L, V, S):
    """oracle.param_specs: the reference's variables and shapes"""
    cfg = do.DalleConfig(d, V - 1 - 16, 16, S // 2, S - S // 2, L, max(1, d // 128))
    assert cfg.total_tokens == V
    return OrderedDict((n, tuple(s[0])) for n, s in do.param_specs(cfg).items())


SIZES = {"dalle_example": (512, 6, 50258 + 512 + 1, 1280), "1.3B": (2048, 24, 50258 + 512 + 1, 1280), "width64": (64, 2, 57, 16)}


@pytest.mark.parametrize("size", sorted(SIZES))
def test_factoring_of_every_reference_variable(size):
    d, L, V, S = SIZES[size]
    lay = ParamLayout(d, L, max(1, d // 128), V, S)
    ref = _reference_shapes(d, L, V, S)
    mine = OrderedDict((n, (shp, off, ld)) for n, shp, off, ld in lay.reference_variables())
    assert sorted(mine) == sorted(ref)          # q / k / v split out of the fused matrix, no "qkv"
    for n, shp in ref.items():
        assert mine[n][0] == shp, n
        assert adafactor_factored_dims(shp) == ar.factored_dims(shp), n
        fd = ar.factored_dims(shp)
        if len(shp) == 1 or d < 128 and min(shp) < 128:
            assert fd is None, n
    if d >= 128:
        for n, shp in ref.items():
            if len(shp) == 2:
                assert ar.factored_dims(shp) is not None, n   # wte, wpe (S = 1280), q/k/v/o, both MLP kernels, head kernel
        assert ar.factored_dims((d, d)) == (0, 1)                 # tie: d0 keeps axis order
        assert ar.factored_dims((d, 4 * d)) == (1, 0)
        assert ar.factored_dims((4 * d, d)) == (0, 1)
        assert ar.factored_dims((V, d)) == (0, 1) and ar.factored_dims((d, V)) == (1, 0)
    else:
        assert all(ar.factored_dims(s) is None for s in ref.values())
    # the fused q|k|v blocks: column blocks of width d of the [d, 3d] matrix; the head keeps V of its Vp columns
    q, k, v = (mine[f"layer_0/attn/{t}"] for t in "qkv")
    assert k[1] - q[1] == d and v[1] - k[1] == d and q[2] == k[2] == v[2] == 3 * d
    assert mine["to_logits/linear_out/kernel"][2] == lay.Vp and mine["to_logits/linear_out/kernel"][0] == (d, V)
    assert ar.factored_dims((512, 2048)) == (1, 0) and ar.factored_dims((512, 512)) == (0, 1)
    assert ar.factored_dims((127, 4096)) is None and ar.factored_dims((128, 4096)) == (1, 0)


@pytest.fixture(scope="module")
def blob():
    z = np.load(FIXTURE)
    return {k: z[k] for k in z.files}


def test_fixture_cases_are_the_generator_cases(blob):
    assert json.loads(str(blob["cases"])) == json.loads(json.dumps(gen.CASES))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


@pytest.mark.parametrize("name", ["a", "b"])
def test_float64_path_reproduces_the_reference_over_shim(blob, name):
    """oracle gradients -> clip -> schedule -> tests/adafactor_ref for three steps == what the reference's own get_optimizer
    computed (case a: decay 0, momentum; case b: decay 0.01, no momentum slot, clip active): variables and every slot"""
    case = gen.CASES[name]
    cfg, weights, tokens = gen.case_inputs(case)
    assert np.array_equal(tokens, blob[name + "/tokens"])
    P, slots, losses = ar.train(weights, tokens, cfg, case["hp"], gen.STEPS, case["step"])
    np.testing.assert_allclose(losses, blob[name + "/loss"], rtol=2e-5)
    after, norms = gen.fixture_case(blob, name)
    assert sorted(after) == sorted(list(P) + list(slots))
    assert (not any(k.endswith("_slot_m") for k in after)) == (case["hp"]["beta_1"] == 0.0)
    assert sorted(norms) == sorted(k for k, v in list(P.items()) + list(slots.items()) if v.size > gen.FULL_MAX)
    for k, v in P.items():
        w0 = gen.sample(weights[k])
        assert _rel(gen.sample(v), after[k]) < 1e-6, (k, _rel(gen.sample(v), after[k]))
        assert _rel(gen.sample(v) - w0, after[k] - w0) < 2e-3, k     # the update itself
        if k in norms:
            assert np.linalg.norm(v - weights[k]) == pytest.approx(norms[k], rel=2e-3), k
    for k, v in slots.items():
        assert after[k].shape == gen.sample(v).shape, k
        assert _rel(gen.sample(v), after[k]) < 1e-4, (k, _rel(gen.sample(v), after[k]))
        if k in norms:
            assert np.linalg.norm(v) == pytest.approx(norms[k], rel=1e-4), k
    factored = [k for k in after if k.endswith("_slot_vr")]
    assert "layer_0/attn/q_slot_vr" in factored and "embedding/wte_slot_vr" in factored
    assert "positional_embedding/wpe_slot_v" in after and "to_logits/linear_out/bias_slot_v" in after


@pytest.mark.skipif(not gen.available(), reason="needs the reference checkout")
def test_fixture_regenerates_identically(tmp_path, monkeypatch):
    monkeypatch.setattr(gen, "OUT", str(tmp_path / "f.npz"))
    gen.main()
    a, b = np.load(FIXTURE), np.load(gen.OUT)
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------- C ABI (nothing launched)
FAKE = ctypes.c_void_p(0x10000)


def _table(rows):
    t = torch.zeros(len(rows), dh.AF_FIELDS, dtype=torch.int64)
    for i, r in enumerate(rows):
        t[i, :len(r)] = torch.tensor(r)
    return t


def test_abi_symbols_declared_and_bound():
    L = dh.lib()
    for name, n in (("dmi_adafactor_plan", 3), ("dmi_adafactor_step", 19)):
        assert name in dh.declared_symbols()
        assert len(getattr(L, name).argtypes) == n
    assert "#define DMI_AF_FIELDS 17" in open(dh.HEADER_PATH).read()


def test_plan_fills_the_table_and_sizes_the_workspace():
    #            off   R    C    ld  fact vr_row row  col  v
    t = _table([[0, 300, 130, 131, 1, 0, 0, 300, 0],
                [40000, 1, 77, 77, 0, 0, 0, 0, 432],
                [40080, 5, 3, 4, 0, 0, 0, 0, 512]])
    tiles, segs, ws = dh.adafactor_plan(t)
    assert tiles == 5 * 1 + 1 + 1
    assert segs == 5 + 3                                            # 64-entry segments of the row and column vectors
    assert t[0, 9] == 0 and t[1, 9] == 5 and t[2, 9] == 6          # tile offsets
    assert t[0, 10] == 5 and t[0, 11] == 1 and t[2, 10] == 1          # row and column tile counts
    assert t[0, 12] == 0 and t[1, 12] == 8 and t[2, 12] == 8       # segment offsets
    assert ws > 4 * (3 * tiles + 300 + 130)


@pytest.mark.parametrize("row,msg", [([0, 0, 4, 4, 0], "bad extents"), ([0, 4, 8, 7, 0], "leading dimension"),
                                     ([0, 4, 4, 4, 2], "factored must be 0 or 1"), ([-4, 4, 4, 4, 0], "bad extents")])
def test_plan_refuses_bad_descriptors(row, msg):
    with pytest.raises(dh.DalleHipError, match=msg):
        dh.adafactor_plan(_table([row]))


def test_step_argument_errors_return_a_status():
    L = dh.lib()
    tot = (ctypes.c_int64 * 3)(7, 3, 4096)

    def call(**kw):
        a = dict(table=FAKE, nv=3, tot=ctypes.addressof(tot), p=FAKE, g=FAKE, m=FAKE, slots=FAKE, pb=None, gn=FAKE, clip=1.0,
                 lr=1e-3, lr_dev=None, decay=0.0, beta1=0.9, eps1=1e-30, eps2=1e-3, ws=FAKE, wsb=4096)
        a.update(kw)
        return L.dmi_adafactor_step(*a.values(), None)
    assert call(p=None) == -1 and "null" in L.dmi_last_error_string().decode()
    assert call(nv=0) == -1
    assert call(wsb=100) == -1 and "workspace" in L.dmi_last_error_string().decode()
    assert call(m=None) == -1 and "momentum" in L.dmi_last_error_string().decode()
    assert call(beta1=1.0) == -1 and call(decay=-0.5) == -1
    assert call(p=ctypes.c_void_p(0x10004)) == -1 and "aligned" in L.dmi_last_error_string().decode()


def test_optim_kernels_use_no_scratch_and_no_spills():
    from dalle_hip import build as b
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([b._hipcc()] + b.FLAGS + ["-I" + os.path.join(ROOT, "include"), "-Rpass-analysis=kernel-resource-usage", "-c",
                            os.path.join(ROOT, "dalle-mtf_amd", "csrc", "optim.hip"), "-o", os.path.join(tmp, "o.o")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout[-2000:]
    usage = {}
    for blk in re.split(r"remark: Function Name: ", p.stdout)[1:]:
        g = lambda k: int(re.search(k + r": (\d+)", blk).group(1))   # noqa: E731
        usage[blk.split()[0]] = dict(scratch=g(r"ScratchSize \[bytes/lane\]"), sgpr_spill=g("SGPRs Spill"), vgpr_spill=g("VGPRs Spill"),
                                     occupancy=g(r"Occupancy \[waves/SIMD\]"))
    assert len([k for k in usage if "af_" in k]) == 6, sorted(usage)
    for k, u in usage.items():
        assert u["scratch"] == 0 and u["vgpr_spill"] == 0 and u["sgpr_spill"] == 0, (k, u)
        assert u["occupancy"] == 8, (k, u)
