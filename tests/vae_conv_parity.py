"""Helpers shared by the layer-level oracle parity tests of the VAE convolutions (tests/test_vae_coco_parity_gpu.py,
tests/test_vae_lowering_gpu.py): seeded bf16 inputs, the bf16 weights as fp32 oracle tensors, and the two checks.  The bounds
describe the rounding of a result to bf16 and the fp32 accumulation order, not a shape:
  * bf16 outputs (forward, input gradients): relative L2 <= 2.1e-3, and every element within 2 bf16 ulp of its value plus 2^-8 of
    the tensor's rms;
  * fp32 outputs (weight / bias gradients, codebook logits): relative L2 <= 1e-5.
Each check notes its figures in the `report` dict it is given."""
import torch


def bf(t):
    return t.to(torch.bfloat16)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return bf(torch.randn(*shape, generator=g) * scale)


def check_bf16(report, name, got, ref):
    got, ref = got.double().flatten(), ref.double().flatten()
    rel = float((got - ref).norm() / ref.norm())
    rms = float(ref.pow(2).mean().sqrt())
    worst = float(((got - ref).abs() - 2.0 ** -7 * ref.abs()).max())     # 2 bf16 ulp of the value
    report[name] = dict(rel_l2=rel, worst_excess_over_2ulp=worst, rms=rms)
    print(name, report[name], flush=True)
    assert rel <= 2.1e-3, (name, rel)
    assert worst <= 2.0 ** -8 * rms, (name, worst, rms)


def check_f32(report, name, got, ref, tol=1e-5):
    got, ref = got.double().flatten(), ref.double().flatten()
    rel = float((got - ref).norm() / ref.norm())
    report[name] = dict(rel_l2=rel)
    print(name, report[name], flush=True)
    assert rel <= tol, (name, rel)


def weights(vae, P, c):
    """the bf16 kernel/bias the product computes with, as fp32 oracle tensors (TF layouts)"""
    k = bf(torch.tensor(P[c.name + "/kernel"])).float().requires_grad_(True)
    b = bf(torch.tensor(P[c.name + "/bias"])).float().requires_grad_(True)
    return k, b
