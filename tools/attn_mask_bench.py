"""Masked attention kernels against the causal ones, alternating in one process (DESIGN.md §4 "Attention masks").
Kernel arms at B = 32, H = 4, S = 1280 (256 text + a 32 x 32 image grid): the causal kernels, the masked kernels on the causal plan
(forced), local:256, row, column and conv:11 -- forward and backward us (median over rounds) and the live-tile fraction.
--step: the dalle_example train step, causal against "row" on every layer.  One JSON line to stdout (and --out FILE)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dalle_hip as dh  # noqa: E402
from src.dalle_mtf.masks import pattern_mask  # noqa: E402


def _time(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) * 1e3 / reps


def kernels(rounds, reps):
    B, H, T, P = 32, 4, 256, 1024
    S = T + P
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = (torch.randn(B * S, 3 * H * 128, device="cuda", generator=g) * 0.35).bfloat16()
    d_o = (torch.randn(B * S, H * 128, device="cuda", generator=g) * 0.5).bfloat16()
    o = torch.empty(B * S, H * 128, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B * H * S, dtype=torch.float32, device="cuda")
    scratch = torch.empty(3 * B * H * S, dtype=torch.float32, device="cuda")
    dqkv = torch.empty_like(qkv)
    arms = {"dense": None, "forced_causal": "causal", "local:256": "local:256", "row": "row", "column": "column", "conv:11": "conv:11"}
    plans = {k: dh.AttnMaskPlan(pattern_mask(v, T, P)) for k, v in arms.items() if v}

    def fwd(k):
        if k == "dense":
            return lambda: dh.attention_fwd(qkv, o, lse, B, H, S)
        return lambda: dh.attention_fwd_masked(qkv, o, lse, plans[k], B, H, S)

    def bwd(k):
        if k == "dense":
            return lambda: dh.attention_bwd(qkv, o, d_o, lse, scratch, dqkv, B, H, S)
        return lambda: dh.attention_bwd_masked(qkv, o, d_o, lse, scratch, dqkv, plans[k], B, H, S)

    res = {k: {"fwd_us": [], "bwd_us": []} for k in arms}
    dh.set_option("attn_mask_force", 1)
    try:
        for k in arms:
            fwd(k)(); bwd(k)()
        torch.cuda.synchronize()
        for _ in range(rounds):
            for k in arms:   # alternating arms
                fwd(k)()
                res[k]["fwd_us"].append(_time(fwd(k), reps))
                res[k]["bwd_us"].append(_time(bwd(k), reps))
    finally:
        dh.set_option("attn_mask_force", 0)
    out = {}
    for k, r in res.items():
        out[k] = dict(fwd_us=float(np.median(r["fwd_us"])), bwd_us=float(np.median(r["bwd_us"])),
                      live_tiles_fwd=plans[k].live_fraction() if k in plans else 1.0,
                      live_tiles_dkv=plans[k].live_fraction_dkv() if k in plans else 1.0)
    d = out["dense"]
    for k, r in out.items():
        r["fwd_vs_dense"] = r["fwd_us"] / d["fwd_us"]
        r["bwd_vs_dense"] = r["bwd_us"] / d["bwd_us"]
    return dict(shape=dict(B=B, H=H, S=S), arms=out)


def step(rounds, steps):
    from oracle import dalle_oracle as do
    from src.dalle_mtf.models import DALLE
    B, T, P = 32, 256, 1024
    tokens = torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, T, 50258, seed=1),
                                                 do.synthetic_image_tokens(B, P, 512, seed=2), 50258)).cuda()
    hp = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
    models = {}
    for name, pat in (("causal", None), ("row", "row")):
        prm = dict(hp, **({"attention_pattern": pat} if pat else {}))
        m = DALLE(n_embd=512, text_vocab_size=50258, image_vocab_size=512, text_seq_len=T, image_seq_len=P, n_layers=6, n_heads=4,
                  batch_size=B, params=prm)
        m.engine.init_params(seed=1234)
        models[name] = m.engine
    res = {k: [] for k in models}
    for eng in models.values():
        for _ in range(2):
            eng.train_step(tokens)
    torch.cuda.synchronize()
    for _ in range(rounds):
        for k, eng in models.items():
            res[k].append(_time(lambda: eng.train_step(tokens), steps) / 1e3)
    out = {k: float(np.median(v)) for k, v in res.items()}
    return dict(step_ms=out, row_vs_causal=out["row"] / out["causal"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args()
    res = step(a.rounds, a.steps) if a.step else kernels(a.rounds, a.reps)
    line = json.dumps(dict(tool="attn_mask_bench", mode="step" if a.step else "kernels", **res))
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
