"""The DALL-E train step with and without text/image loss weights on the MI355X, at the dalle_example dimensions and bench.py's batch
(B = 32): one engine per arm on the same weights and tokens in ONE process, rounds alternating which arm runs first; ms per train step
(median / min / max over the rounds) and a SHA-256 of the unweighted arm's gradients and weights after its first steps.
--tree DIR imports the engine from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.
Usage: python tools/loss_weights_bench.py [--rounds 5] [--iters 10] [--arms plain,weighted] [--tree DIR] [--tag NAME]
       python tools/loss_weights_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
ARMS = {"plain": {}, "weighted": {"text_loss_weight": 1, "image_loss_weight": 7}}


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


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
    if "plain" in engs:      # the unweighted step must compute what the parent commit computes: compare the digests of two trees
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
    print(json.dumps(out), flush=True)


def merge(path, dest):
    """lines tagged "new" (both arms) and "parent" (plain): pooled per arm, in the order they ran"""
    recs = [json.loads(l) for l in open(path) if l.startswith("{")]
    pool = {}
    for r in recs:
        for k, v in r["step_ms"].items():
            pool.setdefault(("parent_" if r["tag"] == "parent" else "") + k, []).append(v["median"])
    digests = {r["tag"]: r.get("plain_digest_after_3_steps") for r in recs}
    out = dict(workload="dalle_example train step, B = 32, one MI355X; per-process medians of alternating rounds, processes of the "
                        "two trees alternating in one call",
               step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
               weighted_minus_plain_ms=statistics.median(pool["weighted"]) - statistics.median(pool["plain"]),
               plain_minus_parent_ms=statistics.median(pool["plain"]) - statistics.median(pool["parent_plain"]),
               plain_digest_after_3_steps=digests, unweighted_bit_identical_to_parent=digests.get("new") == digests.get("parent"))
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    else:
        run(os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            arg("--arms", "plain,weighted").split(","), int(arg("--rounds", 5)), int(arg("--iters", 10)), arg("--tag", "new"))
