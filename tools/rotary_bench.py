"""The DALL-E train step with and without rotary position embeddings on the MI355X, at the dalle_example dimensions and bench.py's
batch (B = 32): one engine per arm on the same weights and tokens in ONE process, rounds alternating which arm runs first; ms per
train step (median / min / max over the rounds), a SHA-256 of the plain arm's gradients, weights and loss after its first three
steps, and dmi_rope_qk alone at the engine's projection buffer ([B S, 3 n_embd] bf16: 4 B per q / k element), forward and inverse,
alternating with dmi_dropout_bwd over as many elements (4 B per element, the bandwidth yardstick).
--tree DIR imports the engine from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.
Usage: python tools/rotary_bench.py [--rounds 5] [--iters 10] [--arms plain,axial] [--tree DIR] [--tag NAME]
       python tools/rotary_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
ARMS = {"plain": {}, "axial": {"rotary_emb": "axial"}, "1d": {"rotary_emb": "1d"}}


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(eng, reps=30):
    """us per launch at the engine's shapes, HIP events around each launch, the kernels alternating"""
    import torch
    import dalle_hip as dh
    M, d, S, H, hd = eng.M, eng.d, eng.S, eng.H, eng.hd
    qkv = torch.randn(M, 3 * d, device=eng.dev).to(torch.bfloat16)
    a, x = (torch.randn(M, 2 * d, device=eng.dev).to(torch.bfloat16) for _ in range(2))
    calls = {"rope_qk": lambda: dh.rope_qk(qkv, eng.rope_cs, M, S, H, hd),
             "rope_qk_inverse": lambda: dh.rope_qk(qkv, eng.rope_cs, M, S, H, hd, inverse=True),
             "dropout_bwd": lambda: dh.dropout_bwd(a, x, M, 2 * d, 0x1234567887654321, 6554)}
    us = {k: [] for k in calls}
    for r in range(reps + 3):
        for k, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    out = {k: summary(v) for k, v in us.items()}
    out["shape"] = [M, 3 * d]
    out["qk_elements"] = M * 2 * d
    for k in calls:
        out[k + "_TB_per_s"] = 4 * M * 2 * d / (out[k]["median"] * 1e-6) / 1e12
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
    rot = [k for k in arms if k != "plain"]
    if rot:
        out["kernels_us"] = kernels(engs[rot[0]])
    print(json.dumps(out), flush=True)


def merge(path, dest):
    """lines tagged "new" (the plain and the rotary arm) and "parent" (plain): pooled per arm, in the order they ran"""
    recs = [json.loads(l) for l in open(path) if l.startswith("{")]
    pool = {}
    for r in recs:
        for k, v in r["step_ms"].items():
            pool.setdefault(("parent_" if r["tag"] == "parent" else "") + k, []).append(v["median"])
    digests = {}
    for r in recs:
        digests.setdefault(r["tag"], []).append(r.get("plain_digest_after_3_steps"))
    kern = [r["kernels_us"] for r in recs if "kernels_us" in r]
    med = lambda k: statistics.median(pool[k])   # noqa: E731
    rot = next(k for k in pool if k not in ("plain", "parent_plain"))
    spread = dict(plain=max(pool["plain"]) - min(pool["plain"]), parent_plain=max(pool["parent_plain"]) - min(pool["parent_plain"]))
    diff = med("plain") - med("parent_plain")
    kmed = {k: statistics.median(r[k]["median"] if isinstance(r[k], dict) else r[k] for r in kern)
            for k in kern[0] if k not in ("shape", "qk_elements")}
    out = dict(workload="dalle_example train step, B = 32, one MI355X; per-process medians of alternating rounds, processes of the "
                        f"two trees alternating in one call; {rot} = rotary_emb {rot!r} (6 + 6 dmi_rope_qk launches per step)",
               step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
               rotary_minus_plain_ms=med(rot) - med("plain"), rotary_over_plain=med(rot) / med("plain"),
               plain_minus_parent_ms=diff, process_spread_ms=spread,
               plain_minus_parent_inside_spread=abs(diff) <= max(spread.values()),
               plain_digest_after_3_steps=digests,
               key_unset_bit_identical_to_parent=len({d for v in digests.values() for d in v}) == 1 and len(digests) == 2,
               kernels_us=dict(median_over_processes=kmed, per_process=kern, shape=kern[0]["shape"], qk_elements=kern[0]["qk_elements"]))
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    else:
        run(os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            arg("--arms", "plain,axial").split(","), int(arg("--rounds", 5)), int(arg("--iters", 10)), arg("--tag", "new"))
