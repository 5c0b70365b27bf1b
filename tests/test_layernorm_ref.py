"""The LayerNorm references of tests/layernorm_ref.py, checked on the CPU: both float32 emulations pass the budget on every family,
the ln_row summation order stays inside half of the derived mean / rstd bounds, within_budget_fwd / within_budget_bwd have teeth -- each
seeded fault is rejected at every width by the family named here -- and the float64 functions agree with torch's layer_norm and
autograd in float64."""
import pytest
import torch
import torch.nn.functional as F

import layernorm_ref as lr

ROWS = 37
D_FWD = [264, 512, 768, 4096]
D_BWD = [264, 512, 768, 2048]
EPS = 1e-5

# the family on which each fault must be rejected at every d (other families may reject it too): named, so that a later edit of the
# families cannot silently lose a fault
REJECTED_BY = {"one_pass_var": "offset1000", "eps_outside": "tiny", "unbiased": "unit", "drop_last_chunk": "offset100",
               "mean_bf16": "offset100", "no_xhat_term": "unit", "dgamma_unscaled": "huge"}

_CACHE = {}


def _fwd(name, d, eps=EPS):
    key = ("f", name, d, eps)
    if key not in _CACHE:
        gamma, beta = lr.params(d, seed=d)
        _CACHE[key] = lr.make_inputs_fwd(lr.families(name, ROWS, d, seed=100 + d), gamma, beta, eps, {name: torch.arange(ROWS)})
    return _CACHE[key]


def _bwd(name, d, dyfam="unit", with_res=True):
    key = ("b", name, d, dyfam, with_res)
    if key not in _CACHE:
        x = lr.families(name, ROWS, d, seed=100 + d)
        gamma, _ = lr.params(d, seed=d)
        g = torch.Generator().manual_seed(7 * d)
        dy = (torch.randn(ROWS, d, generator=g) + (50 if dyfam == "offset" else 0)).to(torch.bfloat16)
        dres = torch.randn(ROWS, d, generator=g).to(torch.bfloat16) if with_res else None
        _, m64, r64 = lr.ln_fwd64(x, gamma, gamma, EPS)
        _CACHE[key] = lr.make_inputs_bwd(dy, x, gamma, m64.float(), r64.float(), dres, {name: torch.arange(ROWS)})
    return _CACHE[key]


@pytest.mark.parametrize("eps", [1e-5, 1e-3])
@pytest.mark.parametrize("d", D_FWD + [8, 64, 1032, 2048])
@pytest.mark.parametrize("name", lr.FAMILIES)
def test_forward_emulations_pass(name, d, eps):
    inp = _fwd(name, d, eps)
    x, g, b = inp["x"], inp["gamma"], inp["beta"]
    r = lr.within_budget_fwd(*lr.emulated_fwd(x, g, b, eps), inp)
    assert r["mean"] <= 0.5 and r["rstd"] <= 0.5, r
    r = lr.within_budget_fwd(*lr.emulated_fwd_lane_order(x, g, b, eps), inp)
    assert r["mean"] <= 0.5 and r["rstd"] <= 0.5, f"the ln_row summation order must leave 2x room under the derived bounds: {r}"


@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("dyfam", ["unit", "offset"])
@pytest.mark.parametrize("d", D_BWD + [8])
@pytest.mark.parametrize("name", lr.FAMILIES)
def test_backward_emulation_passes(name, d, dyfam, with_res):
    inp = _bwd(name, d, dyfam, with_res)
    lr.within_budget_bwd(*lr.emulated_bwd(inp["dy"], inp["x"], inp["gamma"], inp["mean"], inp["rstd"], inp["dres"]), inp)


@pytest.mark.parametrize("d", D_FWD)
@pytest.mark.parametrize("fault", lr.FAULTS_FWD)
def test_forward_faults_are_rejected(fault, d):
    inp = _fwd(REJECTED_BY[fault], d)
    with pytest.raises(AssertionError, match="over its error budget"):
        lr.within_budget_fwd(*lr.emulated_fwd(inp["x"], inp["gamma"], inp["beta"], EPS, fault=fault), inp)


@pytest.mark.parametrize("d", D_BWD)
@pytest.mark.parametrize("fault", lr.FAULTS_BWD)
def test_backward_faults_are_rejected(fault, d):
    inp = _bwd(REJECTED_BY[fault], d)
    got = lr.emulated_bwd(inp["dy"], inp["x"], inp["gamma"], inp["mean"], inp["rstd"], inp["dres"], fault=fault)
    with pytest.raises(AssertionError, match="over its error budget"):
        lr.within_budget_bwd(*got, inp)


def test_a_shifted_constant_row_is_rejected():
    """the constant-row rule: y off beta by one bf16 ulp in one element fails"""
    inp = _fwd("constant", 264)
    y, mean, rstd = lr.emulated_fwd(inp["x"], inp["gamma"], inp["beta"], EPS)
    assert torch.equal(y, inp["beta"].expand_as(y)), "on a constant row a correct fp32 LayerNorm returns beta exactly"
    y = y.clone()
    y[5, 17] = (y[5, 17].double() + lr.ulp_bf16(y[5, 17])).to(torch.bfloat16)
    with pytest.raises(AssertionError, match="constant rows"):
        lr.within_budget_fwd(y, mean, rstd, inp)


@pytest.mark.parametrize("d", [264, 768])
@pytest.mark.parametrize("name", ["unit", "offset100", "rowmix", "one_off"])
def test_float64_functions_agree_with_torch(name, d):
    x = lr.families(name, ROWS, d, seed=d).double().requires_grad_(True)
    gamma, beta = (t.double().requires_grad_(True) for t in lr.params(d, seed=d))
    g = torch.Generator().manual_seed(3)
    dy = torch.randn(ROWS, d, generator=g, dtype=torch.float64)
    eps = lr.eps32(EPS)
    ref = F.layer_norm(x, (d,), gamma, beta, eps)
    ref.backward(dy)
    y, mean, rstd = lr.ln_fwd64(x.detach(), gamma.detach(), beta.detach(), EPS)
    dx, dg, db = lr.ln_bwd64(dy, x.detach(), gamma.detach(), mean, rstd)

    def same(a, b):
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))

    same(y, ref.detach())
    same(dx, x.grad)
    same(dg, gamma.grad)
    same(db, beta.grad)
