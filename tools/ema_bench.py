"""The DALL-E train step with and without the weight EMA on the MI355X, at the dalle_example dimensions and bench.py's batch (B = 32):
one engine per arm on the same weights and tokens in ONE process, rounds alternating which arm runs first; ms per train step
(median / min / max over the rounds), a SHA-256 of the plain arm's gradients, weights and loss after its first three steps, and the
two streaming kernels alone over the engine's flat buffer: dmi_adam_step (30 B per parameter) against dmi_ema_step (14 B).
--tree DIR imports the engine from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.
Usage: python tools/ema_bench.py [--rounds 5] [--iters 10] [--arms plain,ema] [--tree DIR] [--tag NAME]
       python tools/ema_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
ARMS = {"plain": {}, "ema": {"ema_decay": 0.999}}


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(eng, reps=30):
    """us per launch over the engine's n parameters, HIP events around each launch, the two kernels alternating"""
    import torch
    import dalle_hip as dh
    n = eng.lay.total
    ema, eb = torch.zeros_like(eng.p), torch.zeros_like(eng.pb)
    us = {"adam_step": [], "ema_step": []}
    for r in range(reps + 3):
        for k in ("adam_step", "ema_step"):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if k == "adam_step":
                dh.adam_step(eng.p, eng.g, eng.m, eng.v, eng.pb, n, None, 0.0, 0.0, 0.9, 0.999, 1e-6, 0.0)     # lr 0: p stays
            else:
                dh.ema_step(ema, eng.p, eb, n, 1e-3)
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    out = {k: summary(v) for k, v in us.items()}
    out["n"] = n
    out["ema_over_adam"] = out["ema_step"]["median"] / out["adam_step"]["median"]
    out["by_bytes"] = 14.0 / 30.0
    out["ema_TB_per_s"] = 14.0 * n / (out["ema_step"]["median"] * 1e-6) / 1e12
    out["adam_TB_per_s"] = 30.0 * n / (out["adam_step"]["median"] * 1e-6) / 1e12
    return out


def run(tree, arms, rounds, iters, tag):
    for p in (tree, os.path.join(tree, "dalle-mtf_amd")):
        sys.path.insert(0, p)
    import torch
    from bench import MODELS, PER_GPU_BATCH, synth_tokens
    from src.dalle_mtf.engine import DalleEngine
    c = MODELS["dalle_example"]
    B, T, P = PER_GPU_BATCH, c["text_seq_len"], c["image_seq_len"]
    batches = [torch.from_numpy(synth_tokens(B, T, P, c["text_vocab_size"], c["image_vocab_size"], i)).cuda() for i in range(2)]
    engs, out = {}, {"tag": tag, "step_ms": {}}
    for k in arms:
        eng = DalleEngine(c["n_embd"], c["n_layers"], c["n_heads"], c["text_vocab_size"], c["image_vocab_size"], T, P, batch_size=B,
                          global_batch_size=B, hparams=dict(HP, **ARMS[k]))
        eng.init_params(seed=1234)
        eng.global_step = 3000
        engs[k] = eng
    if "plain" in engs:      # the step without the key must compute what the parent commit computes: compare the digests of two trees
        eng = engs["plain"]
        for i in range(3):
            loss = eng.train_step(batches[i % 2])
        torch.cuda.synchronize()
        h = hashlib.sha256(eng.g.cpu().numpy().tobytes() + eng.p.cpu().numpy().tobytes() + loss.cpu().numpy().tobytes())
        out["plain_digest_after_3_steps"] = h.hexdigest()
    st = {k: [] for k in arms}
    for r in range(rounds):
        for k in (arms if r % 2 == 0 else arms[::-1]):
            eng = engs[k]
            for i in range(3):
                eng.train_step(batches[i % 2])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(iters):
                eng.train_step(batches[i % 2])
            torch.cuda.synchronize()
            st[k].append((time.perf_counter() - t0) / iters * 1e3)
    out["step_ms"] = {k: summary(v) for k, v in st.items()}
    if "ema" in engs:
        out["kernels_us"] = kernels(engs["ema"])
    print(json.dumps(out), flush=True)


def merge(path, dest):
    """lines tagged "new" (both arms) and "parent" (plain): pooled per arm, in the order they ran"""
    recs = [json.loads(l) for l in open(path) if l.startswith("{")]
    pool = {}
    for r in recs:
        for k, v in r["step_ms"].items():
            pool.setdefault(("parent_" if r["tag"] == "parent" else "") + k, []).append(v["median"])
    digests = {r["tag"]: r.get("plain_digest_after_3_steps") for r in recs}
    kern = [r["kernels_us"] for r in recs if "kernels_us" in r]
    med = lambda k: statistics.median(pool[k])   # noqa: E731
    out = dict(workload="dalle_example train step, B = 32, one MI355X; per-process medians of alternating rounds, processes of the "
                        "two trees alternating in one call",
               step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
               ema_minus_plain_ms=med("ema") - med("plain"),
               plain_minus_parent_ms=med("plain") - med("parent_plain"),
               process_spread_ms=dict(plain=max(pool["plain"]) - min(pool["plain"]),
                                      parent_plain=max(pool["parent_plain"]) - min(pool["parent_plain"])),
               plain_digest_after_3_steps=digests, key_unset_bit_identical_to_parent=digests.get("new") == digests.get("parent"),
               kernels_us=dict(per_process=kern, ema_over_adam=statistics.median(k["ema_over_adam"] for k in kern), by_bytes=14.0 / 30.0))
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    else:
        run(os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            arg("--arms", "plain,ema").split(","), int(arg("--rounds", 5)), int(arg("--iters", 10)), arg("--tag", "new"))
