"""KL term and codebook statistics of the discrete VAE, CPU side: the float64 specification against closed forms and autograd; the
derived fp32 error bounds of tests/vae_kl_ref.py (they hold for the fp32 restatement in two summation orders, and each seeded fault
falls outside one of them); the config-key resolver and the beta_t schedule; the C ABI (declared, exported, bound; argument errors
come back as a status and a message before anything is launched -- the pointers below are never dereferenced); the compile-time
resources of the new kernels; the statistics arithmetic; and the CPU oracle's confirmation that the KL term lowers the KL."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dalle_hip as dh  # noqa: E402
import vae_kl_ref as ref  # noqa: E402
from src.vae_tf.kl import kl_log_lines, kl_weight_at, resolve_kl_options, usage_stats  # noqa: E402

FAKE = ctypes.c_void_p(0x10000)
DMI_ERR_INVALID = -1
CPU_SHAPES = [(7, 64), (5, 520), (3, 4096)]
TEMPS = (1.0, 0.5, 0.05)
BETAS = (0.5, 6.6)


# ------------------------------------------------------------------ the specification
def test_spec_closed_forms():
    T = 64
    s = ref.kl_spec(np.full((3, T), 0.375, np.float32))
    assert np.allclose(s["q"], 1.0 / T, rtol=1e-15) and np.abs(s["klm"]).max() < 1e-14 and abs(s["kl"]) < 1e-14
    l = np.zeros((1, T), np.float32)
    l[0, 5] = 1000.0                        # one code carries everything: KL = ln T, and no NaN from 0 * (-inf)
    s = ref.kl_spec(l)
    assert np.isfinite(s["e"]).all() and abs(s["kl"] - np.log(T)) < 1e-12
    a, b = ref.kl_spec(ref.family("normal", 4, T)), ref.kl_spec(ref.family("normal", 4, T).astype(np.float64) + 1000.0)
    assert np.allclose(a["klm"], b["klm"], atol=1e-10)


def test_spec_gradient_is_autograd_of_the_loss():
    M, T, beta, tau = 5, 64, 2.0, 0.5
    l = torch.tensor(ref.family("normal", M, T).astype(np.float64), requires_grad=True)
    dy, p = ref.bwd_inputs(M, T, tau, l.detach().numpy())
    lq = torch.log_softmax(l, dim=-1)
    kl = ((lq.exp() * lq).sum(-1) + np.log(T)).mean()
    (beta * kl).backward()
    want = ref.dlogits_spec(np.zeros_like(dy), p, l.detach().numpy(), tau, beta)
    assert np.allclose(l.grad.numpy(), want, rtol=1e-10, atol=1e-16)
    assert abs(float(kl.detach()) - ref.kl_spec(l.detach().numpy())["kl"]) < 1e-12
    # the Gumbel part: d/dz of sum(dy * softmax(z)) at z = l / tau is the existing backward's formula
    z = torch.tensor(np.log(np.maximum(p.astype(np.float64), 1e-300)), requires_grad=True)
    (torch.softmax(z, -1) * torch.tensor(dy.astype(np.float64))).sum().backward()
    pn = torch.softmax(z, -1).detach().numpy()
    got = ref.dlogits_spec(dy, pn, l.detach().numpy(), 1.0, 0.0)
    assert np.allclose(z.grad.numpy(), got, rtol=1e-9, atol=1e-18)


# ------------------------------------------------------------------ the bounds
def _errors(l, tau, beta, order, fault=None):
    """(error, bound) pairs of the fp32 restatement against the float64 specification, by quantity"""
    M, T = l.shape
    s = ref.kl_spec(l)
    rs, kl = ref.kl_fwd_f32(l, order, fault)
    dy, p = ref.bwd_inputs(M, T, tau, l)
    dl = ref.bwd_kl_f32(dy, p, l, ref.kl_fwd_f32(l, order)[0], tau, beta, order, fault)
    out = dict(lse=(np.abs(rs[:, 0] - s["lse"]), ref.lse_bound(l)), e=(np.abs(rs[:, 1] - s["e"]), ref.e_bound(l)),
               kl=(np.abs(kl - s["kl"]), ref.kl_bound(l)),
               dlogits=(np.abs(dl - ref.dlogits_spec(dy, p, l, tau, beta)), ref.dlogits_bound(dy, p, l, tau, beta)),
               qsum=(np.abs(ref.qsum_f32(l, rs, order) - ref.qsum_spec(l)), ref.qsum_bound(l)))
    assert all(np.isfinite(e).all() and np.isfinite(b).all() for e, b in out.values()), (fault, "NaN or Inf")
    return out


@pytest.mark.parametrize("fam", ref.FAMILIES)
def test_bounds_hold_for_the_fp32_restatement_in_two_orders(fam):
    for M, T in CPU_SHAPES:
        l = ref.family(fam, M, T)
        for order in (0, 1):
            for tau, beta in ((1.0, 0.5), (0.5, 6.6), (0.05, 6.6)):
                for name, (err, bound) in _errors(l, tau, beta, order).items():
                    assert (err <= bound).all(), (fam, M, T, order, tau, beta, name, float(np.max(err / bound)))


def test_the_two_orders_differ():
    """(otherwise the test above would show one order twice)"""
    l = ref.family("normal", 7, 4096)
    assert not np.array_equal(ref.kl_fwd_f32(l, 0)[0], ref.kl_fwd_f32(l, 1)[0])


@pytest.mark.parametrize("fault,quantity", [("no_ln_t", "kl"), ("no_e", "dlogits"), ("over_mt", "dlogits"), ("q_at_temp", "dlogits")])
def test_seeded_faults_fall_outside_a_bound(fault, quantity):
    assert fault in ref.FAULTS
    caught = []
    for fam in ref.FAMILIES:
        for M, T in CPU_SHAPES:
            err, bound = _errors(ref.family(fam, M, T), 0.5, 6.6, 0, fault)[quantity]
            if not (err <= bound).all():
                caught.append((fam, M, T))
    assert caught, fault


# ------------------------------------------------------------------ config keys
def test_resolver_accepts():
    assert resolve_kl_options({}) == (0.0, None, False) and resolve_kl_options(None) == (0.0, None, False)
    assert resolve_kl_options(dict(kl_loss_weight=None, kl_anneal_steps=None, codebook_stats=None)) == (0.0, None, False)
    assert resolve_kl_options(dict(kl_loss_weight=0)) == (0.0, None, False)
    assert resolve_kl_options(dict(kl_loss_weight=6.6, kl_anneal_steps=5000, codebook_stats=True)) == (6.6, 5000, True)
    assert resolve_kl_options(dict(kl_loss_weight=np.float32(0.5), kl_anneal_steps=np.int64(3))) == (0.5, 3, False)
    assert resolve_kl_options(dict(codebook_stats=False)).codebook_stats is False
    from collections import defaultdict
    d = defaultdict(lambda: None, codebook_stats=True)         # the shape fetch_model_params returns
    assert resolve_kl_options(d) == (0.0, None, True)


@pytest.mark.parametrize("key,value,other", [
    ("kl_loss_weight", -0.1, {}), ("kl_loss_weight", float("nan"), {}), ("kl_loss_weight", float("inf"), {}),
    ("kl_loss_weight", "1", {}), ("kl_loss_weight", True, {}), ("kl_loss_weight", [1.0], {}),
    ("kl_anneal_steps", 0, dict(kl_loss_weight=1.0)), ("kl_anneal_steps", -3, dict(kl_loss_weight=1.0)),
    ("kl_anneal_steps", 2.5, dict(kl_loss_weight=1.0)), ("kl_anneal_steps", True, dict(kl_loss_weight=1.0)),
    ("kl_anneal_steps", "10", dict(kl_loss_weight=1.0)), ("kl_anneal_steps", 10, {}), ("kl_anneal_steps", 10, dict(kl_loss_weight=0.0)),
    ("codebook_stats", 1, {}), ("codebook_stats", "true", {}), ("codebook_stats", 0.0, {})])
def test_resolver_refuses_naming_the_key(key, value, other):
    with pytest.raises(ValueError, match=key):
        resolve_kl_options(dict(other, **{key: value}))


def test_constructor_refuses_before_any_device_work():
    from src.vae_tf import DiscreteVAE
    with pytest.raises(ValueError, match="kl_loss_weight"):
        DiscreteVAE(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch_size=2, kl_loss_weight=-1.0)
    with pytest.raises(ValueError, match="kl_anneal_steps"):
        DiscreteVAE(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch_size=2, kl_anneal_steps=10)


def test_kl_weight_schedule():
    n, beta = 10, 6.6
    assert kl_weight_at(0, beta, n) == 0.0
    assert kl_weight_at(n // 2, beta, n) == beta * 0.5
    assert kl_weight_at(n, beta, n) == beta and kl_weight_at(n + 1, beta, n) == beta and kl_weight_at(10 ** 9, beta, n) == beta
    assert kl_weight_at(0, beta, None) == beta and kl_weight_at(123, beta) == beta
    assert [kl_weight_at(t, 2.0, 2) for t in range(4)] == [0.0, 1.0, 2.0, 2.0]


def test_log_line_says_what_is_on():
    assert kl_log_lines(resolve_kl_options({}), 2048, 32) == []
    (line,) = kl_log_lines(resolve_kl_options(dict(kl_loss_weight=6.6, kl_anneal_steps=5000)), 2048, 32)
    assert "6.6" in line and "5000" in line and "2048" in line
    (line,) = kl_log_lines(resolve_kl_options(dict(codebook_stats=True)), 2048, 32)
    assert "perplexity_soft" in line and "no KL term" in line


# ------------------------------------------------------------------ statistics arithmetic
def test_usage_stats_on_hand_built_inputs():
    T, M = 64, 640
    st = usage_stats(np.full(T, M / T), np.full(T, M // T), M)
    assert abs(st["perplexity_soft"] - T) < 1e-9 and abs(st["perplexity_hard"] - T) < 1e-9
    assert st["codes_used"] == T and st["codes_used_frac"] == 1.0
    one = np.zeros(T)
    one[17] = M
    st = usage_stats(one, one.astype(np.int32), M)
    assert st["perplexity_soft"] == 1.0 and st["perplexity_hard"] == 1.0 and st["codes_used"] == 1 and st["codes_used_frac"] == 1 / T
    two = np.zeros(T)
    two[[3, 9]] = M / 2
    assert abs(usage_stats(two, two.astype(np.int32), M)["perplexity_hard"] - 2.0) < 1e-12
    l, idx = ref.family("peaked", 50, T), np.arange(50) % 7
    s = ref.stats_spec(l, idx)
    st = usage_stats(ref.qsum_spec(l), ref.counts_spec(idx, T), 50)
    assert all(abs(st[k] - s[k]) < 1e-12 for k in st) and s["codes_used"] == 7


# ------------------------------------------------------------------ C ABI
SYMBOLS = dict(dmi_codebook_kl_workspace_bytes=2, dmi_codebook_kl_fwd=7, dmi_gumbel_softmax_bwd_kl=12, dmi_elbo_loss=6,
               dmi_codebook_usage=9)


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def _fwd(M=8, T=64, ptr=FAKE, ws=FAKE):
    return dh.lib().dmi_codebook_kl_fwd(ptr, ptr, ptr, M, T, ws, None)


def _bwd(M=8, T=64, ptr=FAKE, temperature=1.0, beta=1.0, beta_dev=None):
    return dh.lib().dmi_gumbel_softmax_bwd_kl(ptr, ptr, ptr, ptr, ptr, M, T, temperature, None, beta, beta_dev, None)


def _usage(M=8, T=64, q=(FAKE, FAKE, FAKE), c=(FAKE, FAKE), ws=FAKE):
    return dh.lib().dmi_codebook_usage(q[0], q[1], c[0], q[2], c[1], M, T, ws, None)


def test_entry_points_are_declared_exported_and_bound():
    L = dh.lib()
    declared = dh.declared_symbols()
    for name, nargs in SYMBOLS.items():
        assert name in declared, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        assert fn.restype is (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int), name
    for name in ("codebook_kl_workspace_bytes", "codebook_kl_fwd", "gumbel_softmax_bwd_kl", "elbo_loss", "codebook_usage"):
        assert callable(getattr(dh, name))


def test_workspace_bytes():
    wb = dh.lib().dmi_codebook_kl_workspace_bytes
    assert wb(1, 64) >= 64 * 8 and wb(16384, 2048) >= max(16384, 512 * 2048 * 8) and wb(0, 64) == 0
    assert wb(10 ** 7, 8) >= 10 ** 7        # one KL partial per four rows


@pytest.mark.parametrize("call,prefix", [(_fwd, "codebook_kl_fwd"), (_bwd, "gumbel_bwd_kl"), (_usage, "codebook_usage")])
def test_argument_errors_come_back_as_a_status_and_a_message(call, prefix):
    for kw, word in ((dict(M=0), "M must be positive"), (dict(M=-4), "M must be positive"), (dict(T=12), "multiple of 8"),
                     (dict(T=4104), "at most 4096"), (dict(T=0), "multiple of 8")):
        assert call(**kw) == DMI_ERR_INVALID, (prefix, kw)
        assert _msg().startswith(prefix) and word in _msg(), _msg()
        with pytest.raises(dh.DalleHipError):
            dh._check(call(**kw), prefix)


def test_null_pointers_are_refused():
    assert _fwd(ptr=None) == DMI_ERR_INVALID and _msg().startswith("codebook_kl_fwd") and "null" in _msg()
    assert _fwd(ws=None) == DMI_ERR_INVALID and "null" in _msg()
    assert _bwd(ptr=None) == DMI_ERR_INVALID and _msg().startswith("gumbel_bwd_kl") and "null" in _msg()
    assert _usage(ws=None) == DMI_ERR_INVALID and "null" in _msg()
    assert _usage(q=(None, None, None), c=(None, None)) == DMI_ERR_INVALID and "null" in _msg()      # nothing asked for
    assert _usage(q=(None, FAKE, FAKE)) == DMI_ERR_INVALID and "qsum needs" in _msg()
    assert _usage(q=(FAKE, None, FAKE)) == DMI_ERR_INVALID and "qsum needs" in _msg()
    assert _usage(c=(None, FAKE)) == DMI_ERR_INVALID and "counts needs" in _msg()
    L = dh.lib()
    assert L.dmi_elbo_loss(None, FAKE, 1.0, None, FAKE, None) == DMI_ERR_INVALID and _msg().startswith("elbo_loss")
    assert L.dmi_elbo_loss(FAKE, FAKE, -1.0, None, FAKE, None) == DMI_ERR_INVALID and "kl_weight" in _msg()


def test_by_value_weight_and_temperature_are_checked():
    for beta in (-0.5, float("nan"), float("inf")):
        assert _bwd(beta=beta) == DMI_ERR_INVALID and "kl_weight" in _msg(), beta
    assert _bwd(temperature=0.0) == DMI_ERR_INVALID and "temperature" in _msg()


# ------------------------------------------------------------------ compile-time resources
def test_new_kernels_use_no_scratch_and_have_no_spills():
    import kres
    usage = kres.usage("vae.hip")
    mine = {k: v for k, v in usage.items() if "codebook_kl_fwd_kernel" in k or "gumbel_bwd_kl_kernel" in k or "codebook_usage" in k
            or "elbo_loss_kernel" in k}
    assert len(mine) == 8, sorted(mine)       # four NC instances, the fused backward, the two usage stages, the loss sum
    for k, u in mine.items():
        assert u["scratch"] == 0 and u["vspill"] == 0 and u["sspill"] == 0, (k, u)
    # one wave per row with the whole row in registers: even the 4096-column instance keeps five waves per SIMD
    fwd = [u for k, u in mine.items() if "codebook_kl_fwd_kernel" in k]
    assert len(fwd) == 4 and all(u["occ"] >= 5 for u in fwd), fwd
    assert all(u["occ"] >= 8 for k, u in mine.items() if "codebook_kl_fwd_kernel" not in k), mine
    (part,) = [u for k, u in mine.items() if "codebook_usage_part_kernel" in k]
    assert part["lds"] == 3 * 4096 * 4        # three row groups' sums, then the histogram over the same storage: three slabs per CU


# ------------------------------------------------------------------ the KL term lowers the KL (CPU oracle)
def oracle_kl_curve(case, beta):
    """`steps` Adam steps of the CPU oracle on one batch (soft Gumbel, temperature 1, one noise draw per step) with
    beta * KL(q || uniform) added to the reconstruction loss here, in the test's own code -> the KL before every step"""
    from collections import OrderedDict
    from oracle import vae_oracle as vo
    cfg = vo.VaeConfig(case["num_tokens"], case["dimensions"], case["convblocks"])
    P = vo.init_params(cfg, seed=case["param_seed"])
    img = torch.tensor(vo.synthetic_images(case["batch"], case["dimensions"], seed=case["image_seed"]))
    m = {n: np.zeros_like(a) for n, a in P.items()}
    v = {n: np.zeros_like(a) for n, a in P.items()}
    curve = []
    for step in range(case["steps"] + 1):
        Pt = OrderedDict((n, torch.tensor(a, requires_grad=True)) for n, a in P.items())
        logits = vo.encoder(Pt, img, cfg)
        lq = torch.log_softmax(logits.reshape(-1, case["num_tokens"]), dim=-1)
        kl = ((lq.exp() * lq).sum(-1) + float(np.log(case["num_tokens"]))).mean()
        curve.append(float(kl.detach()))
        if step == case["steps"]:
            break
        u = torch.tensor(vo.synthetic_uniforms(tuple(logits.shape), seed=case["noise_seed"] + step))
        out = vo.decoder(Pt, vo.gumbel_softmax(logits, u, 1.0, hard=False), cfg)
        (vo.mse_loss(img, out) + beta * kl).backward()
        P, m, v = vo.tf_adam_step(P, {n: p.grad.numpy() for n, p in Pt.items()}, m, v, step + 1, case["lr"])
    return curve


def test_oracle_confirms_the_kl_term_lowers_the_kl():
    case = ref.SIGN_CASE
    with_kl = oracle_kl_curve(case, case["beta"])
    assert with_kl[-1] < with_kl[0], with_kl
    without = oracle_kl_curve(case, 0.0)
    assert with_kl[-1] < without[-1], (with_kl[-1], without[-1])      # and it is the term that does it
