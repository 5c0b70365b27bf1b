"""On-device parity harness used by tests/ and __graft_entry__.smoke(): DALL-E train steps through the HIP engine vs the
CPU oracle on identical weights and tokens.  TEST INFRASTRUCTURE: the oracle is imported HERE (checker only); nothing in
the product package imports this file."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "dalle-mtf_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def rel_l2(a, b):
    a = np.asarray(a, np.float64).ravel()
    b = np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def save_report(name, obj):
    """best effort: parity tables land under gpurun_out/ (copied to profiles/ by the author)."""
    try:
        d = os.path.join(ROOT, "gpurun_out")
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, name), "w") as f:
            json.dump(obj, f, indent=1, default=lambda o: float(o) if isinstance(o, (np.floating,)) else str(o))
    except OSError:
        pass


def engine_sites(eng):
    """the activations DalleEngine keeps for its backward, under the oracle's teacher-forcing site names"""
    assert not eng.recompute, "recompute_grad keeps one shared set of block buffers"
    B, S, d, L = eng.B, eng.S, eng.d, eng.L
    f = lambda t, n=None: t.float().cpu().reshape(B, S, -1)
    sites = {"embed": f(eng.X[0]), "xnf": f(eng.xnf)}
    for l in range(L):
        p = f"layer_{l}/"
        qkv = f(eng.qkv[l])
        sites.update({p + "xn1": f(eng.xn1[l]), p + "q": qkv[..., :d].contiguous(), p + "k": qkv[..., d:2 * d].contiguous(),
                      p + "v": qkv[..., 2 * d:].contiguous(), p + "a": f(eng.o[l]), p + "x1": f(eng.x1[l]),
                      p + "xn2": f(eng.xn2[l]), p + "h": f(eng.h[l]), p + "out": f(eng.X[l + 1])})
    return sites


def compare_step(n_embd=256, n_heads=2, n_layers=2, text_vocab=300, image_vocab=64, T=16, P=112, B=2, seed=0,
                 steps=2, verbose=True, hp=None, perturb=0.05, bf16_oracle=True, per_tensor=False, bf16_grad_oracle=False, ref_kw=None):
    """bf16_grad_oracle: also compare against the bf16 oracle with fp32 weight gradients and against the TEACHER-FORCED bf16
    oracle (oracle/dalle_oracle.py _force: forward = the engine's stored activations, backward = the oracle's).
    ref_kw: keywords of tests/dalle_step_ref.py loss_and_grads (e.g. dict(activation="gelu")); the fp32 oracle is then that one, and
    the bf16 oracles, which know no such option, are left out"""
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    cfg = do.DalleConfig(n_embd, text_vocab, image_vocab, T, P, n_layers, n_heads)
    hp = dict(hp or dict(lr=1e-3, train_steps=1000, warmup_steps=2, gradient_clipping=1.0))
    P0 = do.init_params(cfg, seed=1234 + seed, perturb=perturb)
    text = do.synthetic_captions(B, T, text_vocab, seed=seed + 1)
    img = do.synthetic_image_tokens(B, P, image_vocab, seed=seed + 2)
    tokens = do.assemble_tokens(text, img, text_vocab)
    eng = DalleEngine(n_embd, n_layers, n_heads, text_vocab, image_vocab, T, P, batch_size=B, hparams=hp)
    eng.load_reference_params(P0)
    tok_d = torch.from_numpy(tokens).cuda()
    # oracle state
    Po = {k: v.copy() for k, v in P0.items()}
    m = {k: np.zeros_like(v) for k, v in P0.items()}
    v = {k: np.zeros_like(v) for k, v in P0.items()}
    report = {"config": dict(n_embd=n_embd, n_heads=n_heads, n_layers=n_layers, V=cfg.total_tokens, S=T + P, B=B), "steps": []}
    for step in range(steps):
        if ref_kw:
            import dalle_step_ref
            loss_o32, g32 = dalle_step_ref.loss_and_grads(Po, tokens, cfg, **ref_kw)
        else:
            loss_o32, g32 = do.loss_and_grads(Po, tokens, cfg, bf16=False)
        loss_h = float(eng.forward(tok_d, need_grad=True).item())
        eng.backward()
        eng.wait_grads()
        gh = eng.export_reference(eng.g)
        table32 = {k: rel_l2(gh[k], g32[k]) for k in g32}
        worst32 = max(((e, k) for k, e in table32.items()), key=lambda t: t[0])
        rec = dict(step=step, loss_hip=loss_h, loss_oracle_fp32=loss_o32, worst_grad_rel_l2_vs_fp32_oracle=worst32,
                   head_fixup_flag=int(eng.head_flag.item()))
        if bf16_oracle and not ref_kw:
            loss_o16, g16 = do.loss_and_grads(Po, tokens, cfg, bf16=True)
            rec["loss_oracle_bf16"] = loss_o16
            table16 = {k: rel_l2(gh[k], g16[k]) for k in g16}
            rec["worst_grad_rel_l2_vs_bf16_oracle"] = max(((e, k) for k, e in table16.items()), key=lambda t: t[0])
            if per_tensor:
                rec["grad_rel_l2_vs_bf16_oracle"] = table16
        if bf16_grad_oracle and not ref_kw:
            # (a) free-running bf16 oracle whose weight gradients stay fp32 (the engine accumulates them in fp32);
            # (b), (c) TEACHER-FORCED: the oracle's forward takes the activations the engine stored for its own backward, so the
            # forward divergence of two bf16 implementations (rounding-boundary / ReLU-mask flips from different fp32
            # summation orders) is gone and the BACKWARD arithmetic is compared alone
            sites = engine_sites(eng)
            for tag, mode, force in (("bf16_fp32w", "fp32w", None), ("forced_bf16", True, sites), ("forced_fp32w", "fp32w", sites),
                                     ("forced_fp32w_ds", "fp32w+ds", sites),      # "+ds": dS rounded to bf16 as a matrix-core operand
                                     ("forced_fp32w_dp32", "fp32w+dp32", sites),  # "+dp32": dP = dO V^T kept in fp32 (flash-style kernels)
                                     ("forced_fp32w_fa", "fp32w+fa", sites)):     # "+fa": delta = rowsum(dO * O) from the bf16-rounded O
                loss_og, gg = do.loss_and_grads(Po, tokens, cfg, bf16=mode, force=force)
                tab = {k: rel_l2(gh[k], gg[k]) for k in gg}
                rec[f"loss_oracle_{tag}"] = loss_og
                rec[f"worst_grad_rel_l2_vs_{tag}_oracle"] = max(((e, k) for k, e in tab.items()), key=lambda t: t[0])
                if per_tensor:
                    rec[f"grad_rel_l2_vs_{tag}_oracle"] = tab
        gn_h = math.sqrt(sum(float((gh[k].astype(np.float64) ** 2).sum()) for k in gh))
        gn_o = math.sqrt(sum(float((g32[k].astype(np.float64) ** 2).sum()) for k in g32))
        eng.global_step = step + 1  # past step 0 (lr(0) = 0 under warm-up)
        lr = eng.optimizer_step()
        # oracle update with the same schedule position
        gc, _ = do.clip_by_global_norm(g32, hp.get("gradient_clipping", 1.0))
        do.adam_step(Po, gc, m, v, do.learning_rate(step + 1, hp["lr"], hp["train_steps"], hp.get("warmup_steps", 3000)))
        ph = eng.export_reference(eng.p)
        pw = max(((float(np.abs(ph[k] - Po[k]).max()), k) for k in Po), key=lambda t: t[0])
        rec.update(grad_norm_hip=gn_h, grad_norm_oracle=gn_o, lr=lr, worst_param_abs_diff=pw)
        if per_tensor:
            rec["grad_rel_l2"] = table32
        report["steps"].append(rec)
        if verbose:
            print({k: v for k, v in rec.items() if not k.startswith("grad_rel_l2")}, flush=True)
            if per_tensor:
                for k, e in sorted(table32.items(), key=lambda t: -t[1])[:12]:
                    print(f"    rel-L2 {e:.4f}  {k}", flush=True)
    del eng
    torch.cuda.empty_cache()
    return report


def check_report(report, loss_rtol=5e-4, grad_tol=4.8e-2, grad_tol_later=0.092, gn_rtol=2e-3):
    """bf16 compute vs the fp32 oracle: relative loss error, every gradient tensor's relative L2 error on
    the first step (identical weights) and afterwards (weights have drifted by the sign-like first Adam updates), global
    grad-norm.  Defaults = the small smoke configuration's measured values + 25 % (loss 3.7e-5 / 1.5e-4 relative, worst
    gradient tensor 0.038 first step / 0.073 second step, grad norm 4e-4 / 6e-4); the headline-shape tests pass their own
    measured bounds (profiles/r02_parity_*.json hold the tables).
    Parameters: Adam WITHOUT bias correction moves a weight by lr*0.1g/(sqrt(0.001)|g|+eps) ~= 3.16*lr on its first
    step whatever |g| is, so a noise-level gradient whose sign differs costs 2*3.16*lr: bound 6.5*lr per element
    (exactness of the update rule itself on identical gradients is pinned by test_sumsq_adam_cast)."""
    for r in report["steps"]:
        first = r["step"] == 0
        assert abs(r["loss_hip"] - r["loss_oracle_fp32"]) <= loss_rtol * abs(r["loss_oracle_fp32"]), r
        assert r["worst_grad_rel_l2_vs_fp32_oracle"][0] <= (grad_tol if first else grad_tol_later), r
        assert abs(r["grad_norm_hip"] - r["grad_norm_oracle"]) <= gn_rtol * r["grad_norm_oracle"], r
        assert r["worst_param_abs_diff"][0] <= 6.5 * r["lr"] * (1 if first else 2) + 1e-6, r


def smoke_step():
    rep = compare_step()
    check_report(rep)
    print("[smoke] DALL-E train step through libdalle_hip matches the CPU oracle:",
          {k: rep["steps"][-1][k] for k in ("loss_hip", "loss_oracle_fp32", "grad_norm_hip", "grad_norm_oracle")})
