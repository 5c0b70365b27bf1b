"""ReLU against GELU in the DALL-E train step on the MI355X, alternating in one process (same clocks, same box), at the dalle_example
dimensions and bench.py's batch (B = 32): one engine per activation on the same weights and tokens, rounds alternating which runs
first; ms per train step (median / min / max over the rounds).  The per-kernel split comes from a separate
`rocprofv3 --kernel-trace --stats` run of this script with --profile (a few steps of each, no timing): FFN-1 is
gemm_nt8p_kernel<3> (BIAS | RELU) / <1537> (BIAS | GELU | pre), the FFN-2 input gradient gemm_nt8p_kernel<8> (ReLU mask; <256>
with the bit mask) / <2048> (GELU gradient), one launch per layer each; --stats FILE reads such a kernel_stats.csv and prints their
us per layer.  Prints one JSON line, which --out FILE also writes to FILE.
Usage: python tools/act_bench.py [--rounds 5] [--iters 10] [--out FILE]
       rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o act -- python tools/act_bench.py --profile
       python tools/act_bench.py --stats DIR/.../act_kernel_stats.csv [--out FILE]"""
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools"), os.path.join(ROOT, "dalle-mtf_amd")):
    sys.path.insert(0, p)

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
# flag values of the instantiations (csrc/gemm.hip): BIAS 1, RELU 2, RELU_MASK 8, MASK_BITS 256, GELU 512, GELU_PRE 1024, GELU_GRAD 2048
KERNELS = {"relu": {"ffn1": ("<3>", "<131>"), "ffn2_dgrad": ("<8>", "<256>")},
           "gelu": {"ffn1": ("<1537>",), "ffn2_dgrad": ("<2048>",)}}


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def engines():
    import torch
    from bench import MODELS, PER_GPU_BATCH, synth_tokens
    from src.dalle_mtf.engine import DalleEngine
    c = MODELS["dalle_example"]
    out = {}
    for act in ("relu", "gelu"):
        eng = DalleEngine(c["n_embd"], c["n_layers"], c["n_heads"], c["text_vocab_size"], c["image_vocab_size"], c["text_seq_len"],
                          c["image_seq_len"], batch_size=PER_GPU_BATCH, global_batch_size=PER_GPU_BATCH,
                          hparams=dict(HP, activation_fn=act))
        eng.init_params(seed=1234)
        eng.global_step = 3000
        out[act] = eng
    B, T, P = PER_GPU_BATCH, c["text_seq_len"], c["image_seq_len"]
    batches = [torch.from_numpy(synth_tokens(B, T, P, c["text_vocab_size"], c["image_vocab_size"], i)).cuda() for i in range(2)]
    return out, batches, c


def step_times(rounds, iters):
    import torch
    engs, batches, c = engines()
    st = {"relu": [], "gelu": []}
    for r in range(rounds):
        for k in (("relu", "gelu") if r % 2 == 0 else ("gelu", "relu")):
            eng = engs[k]
            for i in range(2):
                eng.train_step(batches[i % 2])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(iters):
                eng.train_step(batches[i % 2])
            torch.cuda.synchronize()
            st[k].append((time.perf_counter() - t0) / iters * 1e3)
    out = {"step_ms": {k: summary(v) for k, v in st.items()}}
    out["gelu_minus_relu_ms"] = out["step_ms"]["gelu"]["median"] - out["step_ms"]["relu"]["median"]
    d, M = c["n_embd"], 32 * (c["text_seq_len"] + c["image_seq_len"])
    # extra HBM bytes per layer: pre written by FFN-1 and read by the FFN-2 input gradient (bf16), in place of the ReLU bit mask
    # written and read; the GELU gradient no longer needs h, which the bit mask already avoided
    out["extra_bytes_per_layer"] = dict(pre_written=2 * M * 4 * d, pre_read=2 * M * 4 * d, relu_bits_written=M * 4 * d // 8,
                                        relu_bits_read=M * 4 * d // 8)
    out["uses_relu_bits"] = engs["relu"].use_relu_bits
    print("train step ms:", {k: (round(v["median"], 3), round(v["min"], 3), round(v["max"], 3)) for k, v in out["step_ms"].items()},
          "GELU - ReLU:", round(out["gelu_minus_relu_ms"], 3), "ms", flush=True)
    return out


def profile_run(steps=5):
    """the run to put under rocprofv3: a few steps of each activation (kernel names carry the flag template argument)"""
    import torch
    engs, batches, _ = engines()
    for k in ("relu", "gelu"):
        for i in range(steps):
            engs[k].train_step(batches[i % 2])
        torch.cuda.synchronize()


def kernel_split(path, n_layers=6, steps=5):
    """us per layer of FFN-1 and the FFN-2 input gradient from a rocprofv3 kernel_stats.csv of profile_run"""
    rows = list(csv.DictReader(open(path)))
    out = {}
    for act, parts in KERNELS.items():
        for part, tags in parts.items():
            hit = [r for r in rows if any(f"gemm_nt8p_kernel{t}(" in r["Name"] for t in tags)]
            calls = sum(int(r["Calls"]) for r in hit)
            total_ns = sum(float(r["TotalDurationNs"]) for r in hit)
            out[f"{act}_{part}"] = dict(kernels=[r["Name"] for r in hit], calls=calls,
                                        us_per_call=(total_ns / calls / 1e3) if calls else None,
                                        expected_calls=n_layers * steps)
    return out


def main():
    if "--profile" in sys.argv:
        profile_run()
        return
    if "--stats" in sys.argv:
        out = {"kernels": kernel_split(sys.argv[sys.argv.index("--stats") + 1])}
    else:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
        iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 10
        out = step_times(rounds, iters)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
