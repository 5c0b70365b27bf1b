"""Plain CPU references of the attention backward and the per-row error budget the tests hold the kernels to.

The kernels take bf16 qkv [B*S, 3, H, hd], the SAVED forward (bf16 o [B*S, H*hd], fp32 lse [B, H, S]) and bf16 d_o [B*S, H*hd];
so do these.  No 1/sqrt(hd): the project folds it into Wq.  mask: bool [S, S], True = attend (None: causal).

  spec64    the formulas in float64, masked entries contributing 0:
              S = Q K^T, P = exp(S - lse), delta = rowsum(dO * O), dP = dO V^T, dS = P * (dP - delta),
              dQ = dS K, dK = dS^T Q, dV = P^T dO
  emulated  the same formulas in float32 with P and dS rounded to bf16 (nearest even) before the three products and dQ, dK, dV
            rounded to bf16 at the end: the arithmetic the header comments of csrc/attention.hip describe.  A model of bf16
            attention backward in general, not of one kernel's loop order -- the yardstick of every bound.
  row_error per (batch, head, row) relative L2 error with a floor, so that a row with a small gradient cannot hide in the tensor's
            largest one
  within_budget  max / median row error of a result against spec64 <= margin * the emulation's own

An `inputs` dict (make_inputs) carries the arguments and caches both references: they are computed once per input set however
many results are judged against them.  Every function returns dq, dk, dv as [B, H, S, hd]."""
import math

import torch

FAULTS = ("diag32", "half_delta", "skip_key64")
# the margins in force at every call site: see the measured table in tests/test_attention_bwd_gpu.py
MARGIN_MAX, MARGIN_MED = 2.0, 1.5


def make_inputs(qkv, o, lse, d_o, B, H, S, hd, mask=None):
    """CPU copies of the kernel arguments; mask: bool [S, S] numpy / torch (True = attend), None = causal"""
    if mask is None:
        m = torch.tril(torch.ones(S, S, dtype=torch.bool))
    else:
        m = torch.as_tensor(mask).cpu().to(torch.bool).clone()
    assert m.shape == (S, S)
    return dict(qkv=qkv.detach().cpu().reshape(B * S, 3 * H * hd), o=o.detach().cpu().reshape(B * S, H * hd),
                lse=lse.detach().cpu().reshape(B, H, S), d_o=d_o.detach().cpu().reshape(B * S, H * hd),
                B=B, H=H, S=S, hd=hd, mask=m)


Q_SCALE = {"flat": 0.12, "warm": 0.5, "peaked": 1.0, "spike": 1.0}
# (keyrow, qrow, mult) of the forward's late-spike tests (S = 1280) scaled down to S = 520: the spiked key in the first tile, in
# steady-state tiles and on the diagonal; qrow % 64 in the lower (70, 389, 140, 519) and the upper (366, 507) 32-row half
SPIKES_520 = [(284, 366, 3.0), (5, 70, 2.0), (261, 366, 3.0), (274, 389, 1.5), (130, 140, 3.0), (519, 519, 3.0), (507, 507, 3.0)]


def family_qkv_do(family, B, H, S, hd, seed, spike=None):
    """bf16 (qkv [B*S, 3*H*hd], d_o [B*S, H*hd]) of an input family: seeded randn, q scaled by Q_SCALE (flat: scores O(1), a nearly
    uniform softmax; peaked: score std ~ sqrt(hd), most rows dominated by one key), d_o of unit scale.  spike = (keyrow, qrow, mult):
    key row keyrow of every (batch, head) set to mult * q[qrow], the way the forward's late-spike tests build theirs."""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B * S, 3, H, hd, generator=g)
    qkv[:, 0] *= Q_SCALE[family]
    d_o = torch.randn(B * S, H * hd, generator=g).to(torch.bfloat16)
    qkv = qkv.to(torch.bfloat16)
    if spike is not None:
        keyrow, qrow, mult = spike
        t = qkv.view(B, S, 3, H, hd)
        t[:, keyrow, 1] = (t[:, qrow, 0].float() * mult).to(torch.bfloat16)
    return qkv.view(B * S, 3 * H * hd), d_o


def forward64(qkv, B, H, S, hd, mask=None):
    """float64 (o [B*S, H*hd], lse [B, H, S]) of masked softmax attention on the bf16 qkv: the saved forward of the CPU tests"""
    m = torch.tril(torch.ones(S, S, dtype=torch.bool)) if mask is None else torch.as_tensor(mask).to(torch.bool)
    q, k, v = split_heads(qkv.double(), B, H, S, hd)
    s = (q @ k.transpose(-1, -2)).masked_fill(~m, float("-inf"))
    lse = torch.logsumexp(s, -1)
    o = torch.exp(s - lse[..., None]) @ v
    return o.permute(0, 2, 1, 3).reshape(B * S, H * hd), lse


def split_heads(dqkv, B, H, S, hd):
    """the kernels' dqkv [B*S, 3, H, hd] -> (dq, dk, dv), each [B, H, S, hd]"""
    t = dqkv.detach().cpu().reshape(B, S, 3, H, hd).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]


def _backward(inp, dtype, bf16_roundings, fault=None):
    B, H, S, hd, mask = inp["B"], inp["H"], inp["S"], inp["hd"], inp["mask"]
    q, k, v = split_heads(inp["qkv"].to(dtype), B, H, S, hd)
    o = inp["o"].to(dtype).view(B, S, H, hd).permute(0, 2, 1, 3)
    d_o = inp["d_o"].to(dtype).view(B, S, H, hd).permute(0, 2, 1, 3)
    lse = inp["lse"].to(dtype)

    def rb(x):
        return x.to(torch.bfloat16).to(dtype) if bf16_roundings else x

    dq, dk, dv = (torch.empty(B, H, S, hd, dtype=dtype) for _ in range(3))
    delta = torch.empty(B, H, S, dtype=dtype)
    idx = torch.arange(S)
    for b in range(B):          # one (batch, head) at a time: the [S, S] intermediates of (8, 16, 1152) at once would be gigabytes
        for h in range(H):
            qi, ki, vi, oi, di = q[b, h], k[b, h], v[b, h], o[b, h], d_o[b, h]
            p = torch.where(mask, torch.exp(qi @ ki.T - lse[b, h][:, None]), torch.zeros((), dtype=dtype))
            dl = (di * oi).sum(-1)
            delta[b, h] = dl
            if fault == "half_delta":       # delta from the first half of the head dimension, doubled
                dl = 2 * (di[:, :hd // 2] * oi[:, :hd // 2]).sum(-1)
            ds = p * (di @ vi.T - dl[:, None])
            if fault == "diag32":           # the diagonal dS element of every 32nd query dropped
                ds[idx[::32], idx[::32]] = 0
            pb, dsb = rb(p), rb(ds)
            dq[b, h] = rb(dsb @ ki)
            dk[b, h] = rb(dsb.T @ qi)
            if fault == "skip_key64":       # the last key of every 64-key chunk skipped, in dV only
                pb = pb.clone()
                pb[:, 63::64] = 0
            dv[b, h] = rb(pb.T @ di)
    return dq, dk, dv, delta


def spec64(inp):
    """(dq, dk, dv, delta) in float64; delta [B, H, S]"""
    return _backward(inp, torch.float64, False)


def emulated(inp, fault=None):
    """(dq, dk, dv, delta) in float32 with the bf16 roundings of a bf16 attention backward.  fault (one of FAULTS) seeds a defect
    of the kind a wrong tile mask / half-row reduction / chunk loop makes: the CPU tests prove within_budget rejects each."""
    assert fault is None or fault in FAULTS
    return _backward(inp, torch.float32, True, fault)


def row_error(got, ref):
    """[B, H, S]: ||got_row - ref_row||_2 / (||ref_row||_2 + floor), floor = 1e-3 * sqrt(head_dim) * rms(ref over that (batch,
    head)), i.e. 1e-3 of the norm a typical row of that head has.  The floor is needed because some reference rows ARE zero: query 0
    has dS = 0 exactly (P = 1, dP = delta), and so has every row one key dominates completely."""
    got, ref = got.double(), ref.double()
    hd = ref.shape[-1]
    rms = ref.pow(2).mean(dim=(-2, -1)).sqrt()
    floor = 1e-3 * math.sqrt(hd) * rms
    return (got - ref).norm(dim=-1) / (ref.norm(dim=-1) + floor[..., None])


def references(inp):
    """(spec64, emulated, {name: row_error(emulated, spec64)}) of an input set, computed once and kept in the dict"""
    if "_refs" not in inp:
        spec, emu = spec64(inp), emulated(inp)
        inp["_refs"] = (spec, emu, {nm: row_error(emu[i], spec[i]) for i, nm in enumerate(("dq", "dk", "dv"))})
    return inp["_refs"]


def within_budget(got, inp, margin_max=MARGIN_MAX, margin_med=MARGIN_MED, label=None):
    """got: the kernels' dqkv [B*S, 3, H, hd] or a (dq, dk, dv[, ...]) tuple of [B, H, S, hd].  Asserts for each of dq, dk, dv
        max row_error(got, spec64)    <= margin_max * max row_error(emulated, spec64)
        median row_error(got, spec64) <= margin_med * median row_error(emulated, spec64)
    and returns {name: (max ratio, median ratio)}; with a label, prints those ratios (got over emulated) before it asserts.  On
    failure prints the worst row, its (batch, head, position) and both values."""
    B, H, S, hd = inp["B"], inp["H"], inp["S"], inp["hd"]
    if torch.is_tensor(got):
        got = split_heads(got, B, H, S, hd)
    spec, _, emu_err = references(inp)
    ratios, failures = {}, []
    for i, nm in enumerate(("dq", "dk", "dv")):
        g = got[i].detach().cpu()
        if not bool(torch.isfinite(g.float()).all()):
            failures.append(f"{nm}: not finite")
            continue
        err, ref = row_error(g, spec[i]), emu_err[nm]
        gmax, gmed, rmax, rmed = float(err.max()), float(err.median()), float(ref.max()), float(ref.median())
        ratios[nm] = (gmax / rmax if rmax > 0 else (0.0 if gmax == 0 else math.inf),
                      gmed / rmed if rmed > 0 else (0.0 if gmed == 0 else math.inf))
        if gmax > margin_max * rmax or gmed > margin_med * rmed:
            w = int(err.argmax())
            pos = (w // (H * S), (w // S) % H, w % S)
            failures.append(f"{nm}: worst row (batch, head, position) = {pos}: row error {gmax:.4g} (emulation there "
                            f"{float(ref[pos]):.4g}); max {gmax:.4g} vs {margin_max} * {rmax:.4g}, "
                            f"median {gmed:.4g} vs {margin_med} * {rmed:.4g}")
    if label is not None:
        print(f"RATIO {label}: " + " | ".join(f"{nm} {r[0]:.3f} {r[1]:.3f}" for nm, r in ratios.items()), flush=True)
    if failures:
        msg = f"attention backward over its error budget at (B, H, S, hd) = {(B, H, S, hd)}:\n  " + "\n  ".join(failures)
        print(msg, flush=True)
        raise AssertionError(msg)
    return ratios
