"""Vector-quantised bottleneck of the discrete VAE, CPU side: the config-key resolver and its log line; the constructor refuses before any
device work; the float64 specification of tests/vae_vq_ref.py is the true gradient (autograd); the input families keep the exact-index
check of the GPU tests from being vacuous; the state-dict rule; the C ABI (declared, exported, bound; argument errors come back as
a status and a message before anything is launched -- the pointers below are never dereferenced); the compile-time resources."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dalle_hip as dh  # noqa: E402
import vae_vq_ref as ref  # noqa: E402
from src.vae_tf.vq import STAT_SCALARS, check_checkpoint, resolve_vq_options, vq_log_lines  # noqa: E402

FAKE = ctypes.c_void_p(0x10000)
DMI_ERR_INVALID, DMI_ERR_UNSUPPORTED = -1, -3
SMALL = dict(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch_size=2)


# ------------------------------------------------------------------ config keys
def test_resolver_accepts():
    off = ("gumbel", None)
    assert resolve_vq_options({}) == off and resolve_vq_options(None) == off
    assert resolve_vq_options(dict(quantizer=None, vq_commitment=None)) == off
    assert resolve_vq_options(dict(quantizer="gumbel")) == off
    assert resolve_vq_options(dict(quantizer="gumbel", kl_loss_weight=2.0, kl_anneal_steps=5)) == off      # the KL keys stay valid when off
    assert resolve_vq_options(dict(quantizer="vq")) == ("vq", 0.25)
    assert resolve_vq_options(dict(quantizer="vq", vq_commitment=0)) == ("vq", 0.0)
    assert resolve_vq_options(dict(quantizer="vq", vq_commitment=np.float32(0.5))) == ("vq", 0.5)
    assert resolve_vq_options(dict(quantizer="vq", vq_commitment=2, codebook_stats=True, kl_loss_weight=0.0)) == ("vq", 2.0)
    from collections import defaultdict
    d = defaultdict(lambda: None, quantizer="vq")         # the shape fetch_model_params returns
    assert resolve_vq_options(d) == ("vq", 0.25)


@pytest.mark.parametrize("key,value,other", [
    ("quantizer", "nearest", {}), ("quantizer", "VQ", {}), ("quantizer", "", {}), ("quantizer", True, {}), ("quantizer", 1, {}),
    ("quantizer", ["vq"], {}),
    ("vq_commitment", -0.1, dict(quantizer="vq")), ("vq_commitment", float("nan"), dict(quantizer="vq")),
    ("vq_commitment", float("inf"), dict(quantizer="vq")), ("vq_commitment", "0.25", dict(quantizer="vq")),
    ("vq_commitment", True, dict(quantizer="vq")), ("vq_commitment", [0.25], dict(quantizer="vq")),
    ("vq_commitment", 0.25, {}), ("vq_commitment", 0.25, dict(quantizer="gumbel")), ("vq_commitment", 0.0, dict(quantizer=None)),
    ("kl_loss_weight", 1.0, dict(quantizer="vq")), ("kl_loss_weight", 1e-9, dict(quantizer="vq")),
    ("kl_anneal_steps", 10, dict(quantizer="vq")), ("kl_anneal_steps", 10, dict(quantizer="vq", kl_loss_weight=1.0, _expect="kl_")),
])
def test_resolver_refuses_naming_the_key(key, value, other):
    other = dict(other)
    match = other.pop("_expect", key)
    with pytest.raises(ValueError, match=match):
        resolve_vq_options(dict(other, **{key: value}))


def test_constructor_refuses_before_any_device_work():
    from src.vae_tf import DiscreteVAE
    with pytest.raises(ValueError, match="quantizer"):
        DiscreteVAE(quantizer="nearest", **SMALL)
    with pytest.raises(ValueError, match="vq_commitment"):
        DiscreteVAE(vq_commitment=0.25, **SMALL)
    with pytest.raises(ValueError, match="vq_commitment"):
        DiscreteVAE(quantizer="vq", vq_commitment=-1.0, **SMALL)
    with pytest.raises(ValueError, match="kl_loss_weight"):
        DiscreteVAE(quantizer="vq", kl_loss_weight=1.0, **SMALL)
    with pytest.raises(ValueError, match="kl_anneal_steps"):
        DiscreteVAE(quantizer="vq", kl_anneal_steps=10, **SMALL)
    for width in (576, 1024):          # a code wider than dmi_vq_assign's rows in LDS: refused here, not at the first forward
        with pytest.raises(ValueError, match="n_hid"):
            DiscreteVAE(quantizer="vq", **dict(SMALL, convblocks=[[1, width]]))


def test_log_line_says_what_is_on():
    assert vq_log_lines(resolve_vq_options({}), 2048, 32, 512) == []
    assert vq_log_lines(resolve_vq_options(dict(quantizer="gumbel")), 2048, 32, 512) == []
    (line,) = vq_log_lines(resolve_vq_options(dict(quantizer="vq", vq_commitment=0.5)), 2048, 32, 512)
    assert "vector quantisation" in line and "0.5" in line and "2048" in line and "512" in line and "temperature" in line
    assert all(k in line for k in STAT_SCALARS) and "loss_vq" in STAT_SCALARS


# ------------------------------------------------------------------ the specification is the true gradient
def _stub_case(unpicked):
    """M = 40, D = 8, T = 6: every code picked at least twice, or code 5 far away from every row"""
    g = np.random.default_rng(11 + unpicked)
    M, D, T = 40, 8, 6
    C = g.standard_normal((T, D))
    if unpicked:
        C[5] = 50.0
    k = np.arange(M) % (T - 1 if unpicked else T)
    X = C[k] + 0.05 * g.standard_normal((M, D))
    W = g.standard_normal((M, D))
    n = np.bincount(ref.assign_spec(X, C)["idx"], minlength=T)
    assert (n[:T - 1] >= 2).all() and (n[5] == 0 if unpicked else n[5] >= 2), n
    return X, C, W


@pytest.mark.parametrize("unpicked", [0, 1])
@pytest.mark.parametrize("beta", [0.25, 0.0, 2.0])
def test_spec_is_autograd_of_the_straight_through_loss(unpicked, beta):
    X, C, W = _stub_case(unpicked)
    gx, gc, d = ref.autograd_grads(X, C, W, beta)
    idx = ref.assign_spec(X, C)["idx"]
    xq = C[idx]
    a = 2.0 * beta / X.size
    assert np.abs(gx - (d + a * (X - xq))).max() <= 1e-12            # ref.dx_spec before its bf16 rounding, beta not rounded to fp32
    want, bound = ref.dc_spec(X, idx, C)
    assert np.abs(gc - want).max() <= 1e-12
    if unpicked:
        assert (gc[5] == 0).all() and (want[5] == 0).all() and (bound[5] == 0).all()
    if beta == 0.25:
        w32, _ = ref.dx_spec(d, X, xq, beta)
        assert np.abs(w32 - gx).max() <= 1e-12
    assert abs(ref.lq_spec(X, xq) - ((X - xq) ** 2).mean()) <= 1e-15


def test_scores_rank_like_distances():
    X, C = ref.family("normal", 50, 64, 64)
    sp = ref.assign_spec(X, C)
    d2 = ((X[:, None, :].astype(np.float64) - C[None].astype(np.float64)) ** 2).sum(-1)
    assert np.array_equal(sp["idx"], d2.argmin(axis=1))
    assert np.allclose(d2, (X.astype(np.float64) ** 2).sum(-1)[:, None] - 2.0 * sp["s"], rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------------ the families
def test_families_are_bf16_valued_and_shaped_as_described():
    for fam in ref.FAMILIES:
        X, C = ref.family(fam, 33, 64, 128)
        assert X.dtype == np.float32 and C.dtype == np.float32 and X.shape == (33, 64) and C.shape == (128, 64)
        assert np.array_equal(ref.round_bf16(X), X) and np.array_equal(ref.round_bf16(C), C), fam
    _, C = ref.family("dup", 5, 64, 128)
    assert np.array_equal(C[64:], C[:64])
    _, C = ref.family("bignorm", 5, 64, 128)
    h = ref.half_norms(C)
    assert h[::7].min() > 20 * np.delete(h, np.arange(0, 128, 7)).max() / 4
    X, C = ref.family("neartie", 40, 64, 128)
    diff = C[1::2] != C[0::2]
    assert (diff.sum(axis=1) >= 1).all() and (diff.sum(axis=1) <= 4).all()
    assert np.allclose(C[1::2][diff], C[0::2][diff], rtol=2.0 ** -6)
    assert (~ref.assign_spec(X, C)["decided"]).any() or (ref.assign_spec(X, C)["gap"] < 1e-2).all()


@pytest.mark.parametrize("D", ref.D_VALUES)
def test_capped_families_leave_few_rows_undecided(D):
    """the exact-index check of the GPU test applies to decided rows only: the float64 reference alone must decide at least 95 % of
    every capped case of the GPU grid, with the seeds of ref.SEEDS"""
    for T in ref.T_VALUES:
        for M in ref.M_VALUES:
            for fam in ref.CAPPED:
                X, C = ref.family(fam, M, D, T)
                sp = ref.assign_spec(X, C)
                assert 1.0 - sp["decided"].mean() <= ref.CAP, (fam, D, T, M, 1.0 - sp["decided"].mean())
                assert sp["bound"].min() > 0 and np.isfinite(sp["bound"]).all()


def test_check_assign_catches_a_wrong_pick():
    X, C = ref.family("normal", 64, 64, 64)
    sp = ref.assign_spec(X, C)
    ref.check_assign(sp, sp["idx"], sp["best"])
    bad = sp["idx"].copy()
    bad[3] = (bad[3] + 1) % 64
    with pytest.raises(AssertionError):
        ref.check_assign(sp, bad)
    with pytest.raises(AssertionError):
        ref.check_assign(sp, sp["idx"], sp["best"] + 1e-3)


# ------------------------------------------------------------------ the state-dict rule (host code)
def test_checkpoint_rule():
    check_checkpoint("gumbel", {"vae_variables": {}})                      # a missing key means Gumbel
    check_checkpoint("gumbel", {"quantizer": None})
    check_checkpoint("vq", {"quantizer": "vq"})
    with pytest.raises(ValueError, match="quantizer"):
        check_checkpoint("vq", {"vae_variables": {}})
    with pytest.raises(ValueError, match="quantizer"):
        check_checkpoint("gumbel", {"quantizer": "vq"})


def test_state_dict_carries_the_key_only_when_on():
    """DiscreteVAE.state_dict / load_state_dict on a stand-in that has the attributes they read: no device needed"""
    from src.vae_tf.models import DiscreteVAE

    class Stub:
        global_step, loaded = 3, None
        m = v = __import__("torch").zeros(4)

        def export_reference(self):
            return {"codebook/codebook": np.zeros((2, 2), np.float32)}

        def load_reference_params(self, P):
            self.loaded = P
    for q in ("gumbel", "vq"):
        s = Stub()
        s.quantizer, s.vq_on = q, q == "vq"
        sd = DiscreteVAE.state_dict(s)
        assert ("quantizer" in sd) == (q == "vq") and sd.get("quantizer", "vq") == "vq"
        DiscreteVAE.load_state_dict(s, sd)
        assert s.loaded is not None and s.global_step == 3
        other = Stub()
        other.quantizer, other.vq_on = ("vq" if q == "gumbel" else "gumbel"), q == "gumbel"
        with pytest.raises(ValueError, match="quantizer"):
            DiscreteVAE.load_state_dict(other, sd)
        assert other.loaded is None


# ------------------------------------------------------------------ C ABI
SYMBOLS = dict(dmi_vq_half_norms=7, dmi_vq_assign=13, dmi_vq_scores_bias=5, dmi_vq_loss_workspace_bytes=0, dmi_vq_loss=9, dmi_vq_bwd_x=12,
               dmi_vq_codebook_grad_workspace_bytes=3, dmi_vq_codebook_grad=11, dmi_vq_gather=9)


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_entry_points_are_declared_exported_and_bound():
    L = dh.lib()
    declared = dh.declared_symbols()
    for name, nargs in SYMBOLS.items():
        assert name in declared, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        assert fn.restype is (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int), name
        assert callable(getattr(dh, name[4:]))
    assert L.dmi_vq_loss_workspace_bytes() >= 1024 * 4 and L.dmi_vq_codebook_grad_workspace_bytes(16384, 2048, 512) >= 0


def _assign(M=8, T=64, D=64, ld=None, x=FAKE, xq=FAKE, h=FAKE):
    ld = D if ld is None else ld
    return dh.lib().dmi_vq_assign(x, ld, FAKE, ld, h, FAKE, xq, ld, FAKE, M, T, D, None)


def test_assign_argument_errors():
    for kw, word in ((dict(M=0), "M must be positive"), (dict(M=-3), "M must be positive"), (dict(x=None), "null"), (dict(h=None), "null"),
                     (dict(ld=60), "ldx"), (dict(D=0), "positive"), (dict(x=ctypes.c_void_p(0x10004)), "aligned")):
        assert _assign(**kw) == DMI_ERR_INVALID and _msg().startswith("vq_assign") and word in _msg(), (kw, _msg())
    for kw in (dict(D=32), dict(D=96), dict(D=576), dict(T=32), dict(T=100), dict(T=4160)):
        assert _assign(**kw) == DMI_ERR_UNSUPPORTED and _msg().startswith("vq_assign"), (kw, _msg())
        with pytest.raises(dh.DalleHipError):
            dh._check(_assign(**kw), "vq_assign")


def test_other_entry_points_refuse_bad_arguments():
    L = dh.lib()
    assert L.dmi_vq_half_norms(FAKE, 64, FAKE, FAKE, 64, 64, None) == DMI_ERR_INVALID and "exactly one" in _msg()
    assert L.dmi_vq_half_norms(None, 64, None, FAKE, 64, 64, None) == DMI_ERR_INVALID and "exactly one" in _msg()
    assert L.dmi_vq_half_norms(FAKE, 64, None, None, 64, 64, None) == DMI_ERR_INVALID and "h" in _msg()
    assert L.dmi_vq_half_norms(FAKE, 1024, None, FAKE, 64, 1024, None) == DMI_ERR_UNSUPPORTED
    assert L.dmi_vq_scores_bias(FAKE, FAKE, 0, 64, None) == DMI_ERR_INVALID and "M must be positive" in _msg()
    assert L.dmi_vq_scores_bias(FAKE, FAKE, 4, 6, None) == DMI_ERR_INVALID and "multiple of 4" in _msg()
    assert L.dmi_vq_scores_bias(None, FAKE, 4, 64, None) == DMI_ERR_INVALID and "null" in _msg()
    assert L.dmi_vq_loss(FAKE, 64, FAKE, 64, FAKE, 4, 64, None, None) == DMI_ERR_INVALID and _msg().startswith("vq_loss") and "null" in _msg()
    assert L.dmi_vq_loss(FAKE, 64, FAKE, 64, FAKE, 0, 64, FAKE, None) == DMI_ERR_INVALID and "M must be positive" in _msg()
    assert L.dmi_vq_loss(FAKE, 64, FAKE, 64, FAKE, 4, 12, FAKE, None) == DMI_ERR_INVALID and "D must be" in _msg()
    assert L.dmi_vq_loss(FAKE, 64, FAKE, 32, FAKE, 4, 64, FAKE, None) == DMI_ERR_INVALID and "ldq" in _msg()
    for beta in (-0.5, float("nan"), float("inf")):
        assert L.dmi_vq_bwd_x(FAKE, 64, FAKE, 64, FAKE, 64, FAKE, 64, 4, 64, beta, None) == DMI_ERR_INVALID and "beta" in _msg(), beta
    assert L.dmi_vq_bwd_x(FAKE, 64, None, 64, FAKE, 64, FAKE, 64, 4, 64, 0.25, None) == DMI_ERR_INVALID and "null" in _msg()
    assert L.dmi_vq_bwd_x(FAKE, 64, FAKE, 64, FAKE, 64, FAKE, 64, 0, 64, 0.25, None) == DMI_ERR_INVALID and "M must be positive" in _msg()
    assert L.dmi_vq_codebook_grad(FAKE, 64, None, FAKE, 64, FAKE, 4, 64, 64, None, None) == DMI_ERR_INVALID and "null" in _msg()
    assert L.dmi_vq_codebook_grad(FAKE, 64, FAKE, FAKE, 64, FAKE, 0, 64, 64, None, None) == DMI_ERR_INVALID and "M must be positive" in _msg()
    assert L.dmi_vq_codebook_grad(FAKE, 1024, FAKE, FAKE, 1024, FAKE, 4, 64, 1024, None, None) == DMI_ERR_UNSUPPORTED
    assert L.dmi_vq_codebook_grad(FAKE, 64, FAKE, FAKE, 64, FAKE, 4, 8192, 64, None, None) == DMI_ERR_UNSUPPORTED
    assert L.dmi_vq_gather(FAKE, 64, None, FAKE, 64, 4, 64, 64, None) == DMI_ERR_INVALID and "null" in _msg()
    assert L.dmi_vq_gather(FAKE, 64, FAKE, FAKE, 64, 0, 64, 64, None) == DMI_ERR_INVALID and "M must be positive" in _msg()
    assert L.dmi_vq_gather(FAKE, 64, FAKE, FAKE, 32, 4, 64, 64, None) == DMI_ERR_INVALID and "ldo" in _msg()


# ------------------------------------------------------------------ compile-time resources
def test_new_kernels_use_no_scratch_and_have_no_spills():
    import kres
    mine = {k: v for k, v in kres.usage("vae.hip").items() if "vq_" in k}
    assert len(mine) == 8, sorted(mine)      # two half-norm forms, assign, scores bias, gather, loss, bwd_x, codebook grad
    for k, u in mine.items():
        assert u["scratch"] == 0 and u["vspill"] == 0 and u["sspill"] == 0, (k, u)
    (assign,) = [u for k, u in mine.items() if "vq_assign_kernel" in k]
    assert assign["vgpr"] + assign["agpr"] <= 256 and assign["occ"] >= 2       # 16 accumulators and both operand sets in registers
    assert all(u["occ"] >= 8 for k, u in mine.items() if "vq_assign_kernel" not in k), mine
