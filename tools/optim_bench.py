"""Adam against Adafactor on the MI355X, alternating in one process (same clocks, same box), at the dalle_example and the 1.3B
dimensions (bench.py's MODELS, imported):
  optimizer alone   Adam path = dmi_sumsq + dmi_adam_step over the flat buffer; Adafactor = dmi_adafactor_step (six launches)
                    -- microseconds, HBM bytes each must move at the least, achieved TB/s
  train step        DalleEngine.train_step at B = 32 with each optimizer (the engine switches its state between rounds)
Adafactor's bytes: g read three times (statistics, x, apply), w twice, m read + written, w written, the bf16 copy written (2 B),
the factored vectors, the full v of the unfactored variables read twice + written; Adam's: g twice (sumsq, step), w, m, v read +
written, bf16 copy.  Prints one JSON line, which --out FILE also writes to FILE.
Usage: python tools/optim_bench.py [--rounds 5] [--models dalle_example,1.3B] [--no-step] [--out FILE]"""
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
from bench import MODELS, PER_GPU_BATCH, synth_tokens  # noqa: E402
from kbench import timeit  # noqa: E402

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def bytes_moved(eng):
    n_real = sum(int(torch.tensor(s).prod()) for _, s, _, _ in eng.lay.reference_variables())
    n_flat = eng.lay.total
    full_v = sum(int(torch.tensor(r["shape"]).prod()) for r in eng.af_vars if not r["factored"])
    vec = sum(sum(r["shape"]) for r in eng.af_vars if r["factored"])
    adam = 4 * n_flat * 2 + 4 * n_flat * 6 + 2 * n_flat                    # g x2; p, m, v read + write; bf16 copy
    ada = 4 * n_real * (3 + 2 + 2 + 1) + 2 * n_real + 4 * full_v * 3 + 4 * vec * 4
    return dict(adam=adam, adafactor=ada, params_flat=n_flat, params_real=n_real, full_v_elems=full_v, vector_elems=vec)


def run_model(name, rounds, step):
    c = MODELS[name]
    from src.dalle_mtf.engine import DalleEngine
    eng = DalleEngine(c["n_embd"], c["n_layers"], c["n_heads"], c["text_vocab_size"], c["image_vocab_size"], c["text_seq_len"],
                      c["image_seq_len"], batch_size=PER_GPU_BATCH, global_batch_size=PER_GPU_BATCH, hparams=dict(HP, optimizer="adafactor"))
    eng.init_params(seed=1234)
    eng.global_step = 3000
    n = eng.lay.total
    eng.g.normal_(0.0, 1e-4)
    am, av = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    gn = torch.zeros(1, device="cuda")

    def adam():
        dh.sumsq(eng.g, n, gn, eng.ws)
        dh.adam_step(eng.p, eng.g, am, av, eng.pb, n, gn, 1.0, 1e-6, 0.9, 0.999, 1e-6, 0.0)

    def ada():
        dh.adafactor_step(eng.af_table, len(eng.af_vars), eng.af_totals, eng.p, eng.g, eng.m, eng.af_slots, eng.pb, gn, 1.0, 1e-6,
                          0.0, 0.9, 1e-30, 1e-3, eng.af_ws)
    t = {"adam": [], "adafactor": []}
    for r in range(rounds):
        for k, fn in ((("adam", adam), ("adafactor", ada)) if r % 2 == 0 else (("adafactor", ada), ("adam", adam))):
            t[k].append(timeit(fn) * 1e6)
    by = bytes_moved(eng)
    out = {"optimizer_us": {k: summary(v) for k, v in t.items()}, "bytes": by}
    out["TBps"] = {k: by[k] / (out["optimizer_us"][k]["median"] * 1e-6) / 1e12 for k in t}
    out["adafactor_over_adam"] = out["optimizer_us"]["adafactor"]["median"] / out["optimizer_us"]["adam"]["median"]
    # optimizer state per GPU (fp32): Adam m + v over the flat buffer; Adafactor m + slots
    out["state_GB"] = {"adam": 2 * 4 * n / 1e9, "adafactor": (4 * n + 4 * eng.af_slots.numel()) / 1e9}
    print(name, "optimizer alone:", {k: round(v["median"], 1) for k, v in out["optimizer_us"].items()}, "us;",
          {k: round(v, 2) for k, v in out["TBps"].items()}, "TB/s; state GB", out["state_GB"], flush=True)
    del am, av
    if step:
        B, T, P = PER_GPU_BATCH, c["text_seq_len"], c["image_seq_len"]
        batches = [torch.from_numpy(synth_tokens(B, T, P, c["text_vocab_size"], c["image_vocab_size"], i)).cuda() for i in range(2)]
        st = {"adam": [], "adafactor": []}
        iters = 10 if c["n_embd"] <= 1024 else 3
        for r in range(rounds):
            for k in (("adam", "adafactor") if r % 2 == 0 else ("adafactor", "adam")):
                eng.set_optimizer(k)
                torch.cuda.empty_cache()
                for i in range(2):
                    eng.train_step(batches[i % 2])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(iters):
                    eng.train_step(batches[i % 2])
                torch.cuda.synchronize()
                st[k].append((time.perf_counter() - t0) / iters * 1e3)
        out["step_ms"] = {k: summary(v) for k, v in st.items()}
        print(name, "train step:", {k: (round(v["median"], 3), round(v["min"], 3), round(v["max"], 3)) for k, v in out["step_ms"].items()},
              flush=True)
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 5
    models = sys.argv[sys.argv.index("--models") + 1].split(",") if "--models" in sys.argv else ["dalle_example", "1.3B"]
    out = {m: run_model(m, rounds, "--no-step" not in sys.argv) for m in models}
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
