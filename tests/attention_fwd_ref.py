"""Plain CPU references of the attention forward / decode and the per-row error budget the tests hold those kernels to: the forward
counterpart of tests/attention_bwd_ref.py, whose input families, float64 forward, row metric and margins it reuses.

The kernels take bf16 qkv [B*S, 3, H, hd] and write bf16 o [B*S, H*hd] and fp32 lse [B, H, S]; so do these.  No 1/sqrt(hd): the
project folds it into Wq.  mask: bool [S, S], True = attend (None: causal).

  forward64         (attention_bwd_ref) masked softmax attention in float64 on the bf16 inputs: the specification
  emulated_forward  the same in float32 with the roundings of a bf16 attention forward: P = exp(s - rowmax) rounded to bf16 (nearest
                    even) before P V, the row sum taken over the UNROUNDED P, o = (P_bf16 V) / sum rounded to bf16, lse = rowmax +
                    log(sum).  A model of bf16 attention forward in general, not of one kernel's loop order -- the yardstick of o.
  lse_bound         a DERIVED worst case per row, 2^-24 * (hd * A + 4 * |lse64| + n + 8) with A = max over the attended keys of
                    sum_d |q_d k_d| and n = the number of attended keys: hd * 2^-24 * A bounds the fp32 accumulation error of one
                    score in any summation order (and an error e of every score moves lse by at most e), n * 2^-24 the relative error
                    of a sum of n non-negative terms in any order (log turns it into an absolute one), the rest is a few ulps of
                    exp, log, and the final add at the magnitude of lse.
  within_budget_fwd max / median row error of o against forward64 <= margin * the emulation's own, |lse - lse64| <= lse_bound

An `inputs` dict (make_inputs) carries the arguments and caches the references: they are computed once per input set however many
results are judged against them."""
import math

import torch

from attention_bwd_ref import MARGIN_MAX, MARGIN_MED, SPIKES_520, family_qkv_do, forward64, row_error, split_heads  # noqa: F401

FAULTS = ("skip_key64", "lse_rounded_sum", "diag_leak")
# half the largest relative error one bf16 rounding can make: no median yardstick is taken smaller than this
MEDIAN_FLOOR = 2.0 ** -10


def _bool_mask(mask, S):
    m = torch.tril(torch.ones(S, S, dtype=torch.bool)) if mask is None else torch.as_tensor(mask).cpu().to(torch.bool).clone()
    assert m.shape == (S, S)
    return m


def make_inputs(qkv, B, H, S, hd, mask=None):
    """CPU copy of the kernel arguments; mask: bool [S, S] numpy / torch (True = attend), None = causal"""
    return dict(qkv=qkv.detach().cpu().reshape(B * S, 3 * H * hd), B=B, H=H, S=S, hd=hd, mask=_bool_mask(mask, S))


def _heads(o, B, H, S, hd):
    """o [B*S, H*hd] -> [B, H, S, hd]"""
    return o.detach().cpu().reshape(B, S, H, hd).permute(0, 2, 1, 3)


def emulated_forward(qkv, B, H, S, hd, mask=None, fault=None):
    """(o bf16 [B*S, H*hd], lse fp32 [B, H, S]) in float32 with the bf16 roundings of a bf16 attention forward (module docstring).
    fault (one of FAULTS) seeds a defect of the kind a wrong chunk loop / reduction / mask makes:
      skip_key64       the last key of every 64-key chunk dropped from P V only (the sum untouched)
      lse_rounded_sum  lse from the sum of the bf16-ROUNDED P
      diag_leak        key i + 1 admitted for every query i = 31 (mod 32)
    The CPU tests prove within_budget_fwd rejects each."""
    assert fault is None or fault in FAULTS
    m = _bool_mask(mask, S)
    if fault == "diag_leak":
        i = torch.arange(31, S - 1, 32)
        m[i, i + 1] = True
    q, k, v = split_heads(qkv.float(), B, H, S, hd)
    o = torch.empty(B, H, S, hd, dtype=torch.bfloat16)
    lse = torch.empty(B, H, S, dtype=torch.float32)
    for b in range(B):              # one (batch, head) at a time: the [S, S] intermediates stay small
        for h in range(H):
            s = (q[b, h] @ k[b, h].T).masked_fill(~m, float("-inf"))
            mx = s.max(-1).values
            p = torch.exp(s - mx[:, None])
            total = p.sum(-1)
            pb = p.to(torch.bfloat16).float()
            lse[b, h] = mx + torch.log(pb.sum(-1) if fault == "lse_rounded_sum" else total)
            if fault == "skip_key64":
                pb[:, 63::64] = 0
            o[b, h] = ((pb @ v[b, h]) / total[:, None]).to(torch.bfloat16)
    return o.permute(0, 2, 1, 3).reshape(B * S, H * hd), lse


def lse_bound(qkv, lse64, B, H, S, hd, mask):
    """[B, H, S] float64: the derived worst case of |lse - lse64| for an fp32 computation of lse (module docstring)"""
    m = _bool_mask(mask, S)
    q, k, _ = split_heads(qkv.double(), B, H, S, hd)
    A = torch.empty(B, H, S, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            A[b, h] = (q[b, h].abs() @ k[b, h].abs().T).masked_fill(~m, 0.0).max(-1).values
    n = m.sum(-1).double()
    return 2.0 ** -24 * (hd * A + 4 * lse64.double().abs() + n + 8)


def references(inp):
    """(o64 [B, H, S, hd], lse64 [B, H, S], emulated o, emulated lse, lse bound, pure rounding bf16(o64)), computed once and kept"""
    if "_refs" not in inp:
        qkv, B, H, S, hd, mask = (inp[k] for k in ("qkv", "B", "H", "S", "hd", "mask"))
        o64, lse64 = (torch.cat(t) for t in zip(*(forward64(qkv.view(B, S, -1)[b], 1, H, S, hd, mask) for b in range(B))))
        eo, el = emulated_forward(qkv, B, H, S, hd, mask)
        o64 = _heads(o64, B, H, S, hd)
        inp["_refs"] = (o64, lse64, _heads(eo, B, H, S, hd), el, lse_bound(qkv, lse64, B, H, S, hd, mask),
                        o64.to(torch.bfloat16))
    return inp["_refs"]


def _ratio(a, b):
    return a / b if b > 0 else (0.0 if a == 0 else math.inf)


def within_budget_fwd(o, lse, inp, margin_max=MARGIN_MAX, margin_med=MARGIN_MED, rows=None, label=None):
    """o: bf16 [B*S, H*hd], lse: fp32 [B, H, S] -- or, with rows = a list of positions, o [B*R, H*hd] and lse [B, H, R] holding those
    positions only (decode hands over some rows and lse=None).  Asserts that everything is finite and
        max row_error(o, o64)    <= margin_max * max row_error(emulated o, o64)
        median row_error(o, o64) <= margin_med * median row_error(emulated o, o64), both medians taken no smaller than MEDIAN_FLOOR
        |lse - lse64|            <= lse_bound on every row
    over the judged rows, and returns dict(emu=(max, median ratio), rounding=(the same against bf16(o64)), lse=worst error / bound);
    with a label, prints those as a RATIO line before it asserts.  On failure names the worst row by (batch, head, position)."""
    B, H, S, hd = inp["B"], inp["H"], inp["S"], inp["hd"]
    o64, lse64, eo, _, bound, pure = references(inp)
    pos = torch.arange(S) if rows is None else torch.as_tensor(list(rows), dtype=torch.long)
    R = len(pos)
    failures, out = [], {}
    g = _heads(o, B, H, R, hd)
    if not bool(torch.isfinite(g.float()).all()):
        failures.append("o: not finite")
    else:
        ref = o64[:, :, pos]
        err, emu, rnd = row_error(g, ref), row_error(eo[:, :, pos], ref), row_error(pure[:, :, pos], ref)
        gmax, gmed = float(err.max()), max(float(err.median()), MEDIAN_FLOOR)
        emax, emed = float(emu.max()), max(float(emu.median()), MEDIAN_FLOOR)
        out["emu"] = (_ratio(gmax, emax), gmed / emed)
        out["rounding"] = (_ratio(gmax, float(rnd.max())), gmed / max(float(rnd.median()), MEDIAN_FLOOR))
        if gmax > margin_max * emax or gmed > margin_med * emed:
            w = int(err.argmax())
            at = (w // (H * R), (w // R) % H, w % R)
            failures.append(f"o: worst row (batch, head, position) = {(at[0], at[1], int(pos[at[2]]))}: row error {gmax:.4g} "
                            f"(emulation there {float(emu[at]):.4g}); max {gmax:.4g} vs {margin_max} * {emax:.4g}, "
                            f"median {gmed:.4g} vs {margin_med} * {emed:.4g}")
    if lse is not None:
        ls = lse.detach().cpu().reshape(B, H, R)
        if not bool(torch.isfinite(ls).all()):
            failures.append("lse: not finite")
        else:
            lerr, lb = (ls.double() - lse64[:, :, pos]).abs(), bound[:, :, pos]
            out["lse"] = float((lerr / lb).max())
            if not bool((lerr <= lb).all()):
                w = int((lerr / lb).argmax())
                at = (w // (H * R), (w // R) % H, w % R)
                failures.append(f"lse: worst row (batch, head, position) = {(at[0], at[1], int(pos[at[2]]))}: |lse - lse64| = "
                                f"{float(lerr[at]):.4g} vs bound {float(lb[at]):.4g} ({out['lse']:.3g} x)")
    if label is not None:
        parts = []
        if "emu" in out:
            parts.append("o/emulation {:.3f} {:.3f} | o/rounding {:.3f} {:.3f}".format(*out["emu"], *out["rounding"]))
        if "lse" in out:
            parts.append(f"lse/bound {out['lse']:.3g}")
        print(f"RATIO {label}: " + " | ".join(parts), flush=True)
    if failures:
        msg = f"attention forward over its error budget at (B, H, S, hd) = {(B, H, S, hd)}:\n  " + "\n  ".join(failures)
        print(msg, flush=True)
        raise AssertionError(msg)
    return out
