"""The FP8 key/value cache measured in one process (random data / weights):
  kernels   dmi_attention_decode against dmi_attention_decode_kv8, head dim 128, at (B, H, S) = (128, 8, 1280) and (32, 4, 1280) and
            positions 256, 768, 1279, alternating per round.  Each call takes the next of several cache copies (together over 1 GB, four
            times the Infinity Cache), as the sampler's layers do: a hot loop over one small cache would time the cache, not HBM.
  loglik    dalle_example at B = 32: one teacher-forced batch decoded on the bf16 and on the fp8 cache, the per-token
            |difference of log p(token)| over the image positions (mean and worst)
Usage: python tools/kv8_bench.py [--rounds 5] [--no-loglik] [--out FILE]"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "dalle-mtf_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import dalle_hip as dh  # noqa: E402
from kbench import rb, timeit  # noqa: E402

HD = 128
SHAPES = [(128, 8, 1280), (32, 4, 1280)]
POSITIONS = [256, 768, 1279]


def kernel_arms(B, H, S):
    d = H * HD
    n16 = max(2, -(-(1 << 30) // (B * S * 3 * d * 2)))
    n8 = max(2, -(-(1 << 30) // (B * S * (2 * d + 8 * H))))
    c16 = [rb(B * S, 3 * d, scale=0.3) for _ in range(n16)]
    c8 = []
    for i in range(n8):
        data = torch.empty(B, S, 2, H, HD, dtype=torch.uint8, device="cuda")
        scale = torch.empty(B, S, 2, H, dtype=torch.float32, device="cuda")
        dh.kv8_quantize(c16[i % n16], data, scale, B, S, H, HD, 0, S)
        c8.append((data, scale))
    fresh = rb(B, 3 * d, scale=0.3)
    o = torch.empty(B, d, dtype=torch.bfloat16, device="cuda")
    it = {"bf16": 0, "fp8": 0}

    def bf16(pos):
        it["bf16"] += 1
        dh.attention_decode(c16[it["bf16"] % n16], o, B, H, S, pos, fresh=fresh, head_dim=HD)

    def fp8(pos):
        it["fp8"] += 1
        dh.attention_decode_kv8(*c8[it["fp8"] % n8], fresh, o, B, H, S, pos, head_dim=HD)

    return {"bf16": bf16, "fp8": fp8}, dict(bf16_copies=n16, fp8_copies=n8)


def kernels(rounds):
    out = {}
    for B, H, S in SHAPES:
        arms, info = kernel_arms(B, H, S)
        for pos in POSITIONS:
            t = {k: [] for k in arms}
            for r in range(rounds):
                for k in (list(arms) if r % 2 == 0 else reversed(list(arms))):
                    t[k].append(timeit(lambda: arms[k](pos)) * 1e6)
            med = {k: statistics.median(v) for k, v in t.items()}
            share = (HD + 4) / (2 * HD)
            row = dict(info, us={k: dict(median=round(med[k], 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in t.items()},
                       fp8_over_bf16=round(med["fp8"] / med["bf16"], 4), byte_share=round(share, 4),
                       target_at_1279=round(1.25 * share, 4))
            out[f"B{B}_H{H}_S{S}_pos{pos}"] = row
            print(f"B {B} H {H} pos {pos}: bf16 {med['bf16']:.1f} us  fp8 {med['fp8']:.1f} us  ratio {row['fp8_over_bf16']:.3f} "
                  f"(bytes {share:.3f})", flush=True)
        del arms
        torch.cuda.empty_cache()
    return out


def loglik():
    from oracle import dalle_oracle as do
    from src.dalle_mtf.engine import DalleEngine
    B, T, P, tv, iv = 32, 256, 1024, 50258, 512
    eng = DalleEngine(512, 6, 4, tv, iv, T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10))
    eng.init_params(seed=1)
    tok = torch.from_numpy(do.assemble_tokens(do.synthetic_captions(B, T, tv, seed=1), do.synthetic_image_tokens(B, P, iv, seed=2), tv)).cuda()
    lp = {}
    for kv in ("bf16", "fp8"):
        with eng.kv_cache_as(kv):
            eng._prefill(tok)
            rows = []
            for pos in range(T - 1, T + P - 1):
                z = eng.decode_step(tok[:, pos].contiguous(), pos, graph=True)
                rows.append(torch.log_softmax(z.float(), -1).gather(1, (tok[:, pos + 1] - tv).long()[:, None])[:, 0])
            lp[kv] = torch.stack(rows, 1).double()
    diff = (lp["fp8"] - lp["bf16"]).abs()
    res = dict(tokens=int(diff.numel()), mean_abs_dloglik_per_token=float(diff.mean()), worst_abs_dloglik_per_token=float(diff.max()),
               mean_loglik_per_token_bf16=float(lp["bf16"].mean()), mean_loglik_per_token_fp8=float(lp["fp8"].mean()))
    print("loglik:", res, flush=True)
    return res


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    out = {"device": torch.cuda.get_device_name(0), "decode_kernels": kernels(rounds)}
    if "--no-loglik" not in sys.argv:
        out["loglik_dalle_example_B32"] = loglik()
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
