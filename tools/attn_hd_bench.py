"""Attention forward / backward by head dimension, three arms timed alternately in one process (same clocks, same box):
  (a) head dim 64,  B = 32, H = 8, S = 1280      -- n_embd 512 with 8 heads
  (b) head dim 128, B = 32, H = 8, S = 1280      -- what zero-padding every 64-wide head to 128 would cost at the least
  (c) head dim 128, B = 32, H = 4, S = 1280      -- the same n_embd and the same flops as (a)
then the dalle_example train step at B = 32 with n_heads = 8 against n_heads = 4 (alternating engines).  Prints medians and spreads
(min..max over the rounds) and one JSON line, which --out FILE also writes to FILE.
Usage: python tools/attn_hd_bench.py [--rounds 5] [--no-step] [--out FILE]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "dalle-mtf_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import dalle_hip as dh  # noqa: E402
from kbench import rb, timeit  # noqa: E402

B, S = 32, 1280
ARMS = {"a_hd64_H8": (64, 8), "b_hd128_H8": (128, 8), "c_hd128_H4": (128, 4)}


def attn_arm(hd, H):
    d = H * hd
    qkv = rb(B * S, 3 * d, scale=0.3)
    o = torch.empty(B * S, d, dtype=torch.bfloat16, device="cuda")
    lse = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
    d_o = rb(B * S, d)
    delta = torch.empty(3, B, H, S, dtype=torch.float32, device="cuda")
    dqkv = torch.empty(B * S, 3 * d, dtype=torch.bfloat16, device="cuda")
    fwd = lambda: dh.attention_fwd(qkv, o, lse, B, H, S, head_dim=hd)   # noqa: E731
    bwd = lambda: dh.attention_bwd(qkv, o, d_o, lse, delta, dqkv, B, H, S, head_dim=hd)   # noqa: E731
    return fwd, bwd


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    fns = {k: attn_arm(*v) for k, v in ARMS.items()}
    t = {k: {"fwd": [], "bwd": []} for k in ARMS}
    for r in range(rounds):
        for k, (fwd, bwd) in (fns.items() if r % 2 == 0 else reversed(list(fns.items()))):
            t[k]["fwd"].append(timeit(fwd) * 1e6)
            t[k]["bwd"].append(timeit(bwd) * 1e6)
    out = {"attention_us": {k: {p: summary(v) for p, v in x.items()} for k, x in t.items()}}
    for k, x in out["attention_us"].items():
        print(f"{k:12s} fwd {x['fwd']['median']:7.1f} us ({x['fwd']['min']:.1f}..{x['fwd']['max']:.1f})   "
              f"bwd {x['bwd']['median']:7.1f} us ({x['bwd']['min']:.1f}..{x['bwd']['max']:.1f})", flush=True)
    a, b, c = (out["attention_us"][k] for k in ARMS)
    out["ratios"] = {f"{p}_a_over_{n}": a[p]["median"] / y[p]["median"] for p in ("fwd", "bwd") for n, y in (("b", b), ("c", c))}
    print("ratios:", {k: round(v, 3) for k, v in out["ratios"].items()}, flush=True)
    del fns
    torch.cuda.empty_cache()

    if "--no-step" not in sys.argv:
        from oracle import dalle_oracle as do
        from src.dalle_mtf.engine import DalleEngine
        hp = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
        batches = [torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, 256, 50258, seed=2 * i + 1),
                                                       do.synthetic_image_tokens(B, 1024, 512, seed=2 * i + 2), 50258)).cuda() for i in range(2)]
        steps = {}
        for heads in (8, 4):
            eng = DalleEngine(512, 6, heads, 50258, 512, 256, 1024, batch_size=B, global_batch_size=B, hparams=hp)
            eng.init_params(seed=1234)
            eng.global_step = 3000
            steps[heads] = eng
        st = {8: [], 4: []}
        for r in range(rounds):
            for heads in ((8, 4) if r % 2 == 0 else (4, 8)):
                eng = steps[heads]
                for i in range(3):
                    eng.train_step(batches[i % 2])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(10):
                    eng.train_step(batches[i % 2])
                torch.cuda.synchronize()
                st[heads].append((time.perf_counter() - t0) / 10 * 1e3)
        out["step_ms"] = {f"n_heads_{h}": summary(v) for h, v in st.items()}
        print("dalle_example step, B = 32:", {k: (round(v["median"], 3), round(v["min"], 3), round(v["max"], 3)) for k, v in out["step_ms"].items()}, flush=True)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
