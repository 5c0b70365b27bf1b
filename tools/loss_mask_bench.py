"""The DALL-E train step with and without "loss_ignore_padding" on the MI355X, at the dalle_example dimensions and bench.py's batch
(B = 32, bench.py's synthetic right-padded captions): one engine per arm on the same weights and tokens in ONE process, rounds
alternating which arm runs first; ms per train step (median / min / max over the rounds) and a SHA-256 of the plain arm's loss,
gradients and weights after its first three steps.
Arms: plain (no loss key), weighted (weights (1, 7)), masked (weights (1, 7) and the key).
--tree DIR imports the engine from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree's processes and the parent's; --kernels times the two new launches and dmi_loss_reduce alone at
M = 32 * 1280 = 40960 with HIP events in one process; --merge joins the JSON lines of such runs into one file.
Usage: python tools/loss_mask_bench.py [--rounds 5] [--iters 10] [--arms plain,weighted,masked] [--tree DIR] [--tag NAME]
       python tools/loss_mask_bench.py --kernels
       python tools/loss_mask_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
W17 = {"text_loss_weight": 1, "image_loss_weight": 7}
ARMS = {"plain": {}, "weighted": W17, "masked": dict(W17, loss_ignore_padding=True)}
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    if "plain" in engs:      # the step without the key must compute what the parent commit computes: compare the digests of two trees
        eng = engs["plain"]
        for i in range(3):
            loss = eng.train_step(batches[i % 2])
        torch.cuda.synchronize()
        h = hashlib.sha256(eng.g.cpu().numpy().tobytes() + eng.p.cpu().numpy().tobytes() + loss.cpu().numpy().tobytes())
        out["plain_digest_after_3_steps"] = h.hexdigest()
    if "masked" in engs:     # the share of the caption labels (tokens 1 .. T - 1) that are not padding, per batch
        out["text_kept_frac"] = [float((b[:, 1:T] != c["text_vocab_size"] - 1).float().mean()) for b in batches]
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


def kernels(tag):
    """us per launch of dmi_loss_mask, dmi_loss_reduce_masked and dmi_loss_reduce at the bench's M, each the median of 200 event-timed
    launches after 20 warm ones, in one process"""
    for p in (HERE, os.path.join(HERE, "dalle-mtf_amd")):
        sys.path.insert(0, p)
    import numpy as np
    import torch
    import dalle_hip as dh
    from bench import MODELS, PER_GPU_BATCH, synth_tokens
    c = MODELS["dalle_example"]
    B, T, P = PER_GPU_BATCH, c["text_seq_len"], c["image_seq_len"]
    S, M, pad = T + P, PER_GPU_BATCH * (T + P), c["text_vocab_size"] - 1
    tok = synth_tokens(B, T, P, c["text_vocab_size"], c["image_vocab_size"], 0)
    labels = torch.from_numpy(np.concatenate([tok[:, 1:], np.full((B, 1), pad + 1, np.int32)], 1)).cuda().contiguous()
    rows = (torch.rand(M) * 9 + 0.05).cuda()
    row_w, counts = torch.zeros(M, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    out4, out3, pw = torch.zeros(4, device="cuda"), torch.zeros(3, device="cuda"), torch.full((S,), 1.0 / S, device="cuda")
    calls = {"dmi_loss_mask": lambda: dh.loss_mask(labels, M, S, T - 1, pad, 0.125, 0.875, False, counts, row_w),
             "dmi_loss_reduce_masked": lambda: dh.loss_reduce_masked(rows, row_w, labels, M, S, T - 1, pad, counts, 1.0, out4),
             "dmi_loss_reduce": lambda: dh.loss_reduce(rows, M, pw, S, T - 1, 1.0 / B, out3)}
    res = {}
    for name, f in calls.items():
        for _ in range(20):
            f()
        us = []
        for _ in range(200):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        res[name] = summary(us)
    print(json.dumps({"tag": tag, "M": M, "kernel_us": res, "counts": counts.tolist()}), flush=True)


def merge(path, dest):
    """lines tagged "new" (three arms), "parent" (plain) and "kernels": per-process medians pooled per arm, in the order they ran.
    spread = max - min of the parent's per-process medians; the key unset is judged against it, the key on against it plus the two
    new launches' own times, measured against the weighted arm of the same processes"""
    recs = [json.loads(l) for l in open(path) if l.startswith("{")]
    pool = {}
    for r in recs:
        for k, v in r.get("step_ms", {}).items():
            pool.setdefault(("parent_" if r["tag"] == "parent" else "") + k, []).append(v["median"])
    digests = {r["tag"]: r.get("plain_digest_after_3_steps") for r in recs if "plain_digest_after_3_steps" in r}
    kern = next((r for r in recs if "kernel_us" in r), None)
    med = {k: statistics.median(v) for k, v in pool.items()}
    spread = max(pool["parent_plain"]) - min(pool["parent_plain"])
    per_proc = [m - w for m, w in zip(pool["masked"], pool["weighted"])]
    out = dict(workload="dalle_example train step, B = 32, one MI355X, bench.py's synthetic right-padded captions; per-process medians "
                        "of alternating rounds, processes of the two trees alternating in one call",
               step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
               text_kept_frac=next((r["text_kept_frac"] for r in recs if "text_kept_frac" in r), None),
               parent_process_spread_ms=spread,
               plain_minus_parent_ms=med["plain"] - med["parent_plain"],
               key_unset_within_parent_spread=abs(med["plain"] - med["parent_plain"]) <= spread,
               plain_digest_after_3_steps=digests, key_unset_bit_identical_to_parent=digests.get("new") == digests.get("parent"),
               masked_minus_weighted_ms=dict(median=med["masked"] - med["weighted"], per_process=per_proc))
    if kern is not None:
        k = kern["kernel_us"]
        new_ms = (k["dmi_loss_mask"]["median"] + k["dmi_loss_reduce_masked"]["median"]) / 1e3
        out.update(kernel_us_at_M=dict(M=kern["M"], **k), new_launches_ms=new_ms, masked_margin_ms=spread + new_ms,
                   key_on_within_margin=med["masked"] - med["weighted"] <= spread + new_ms)
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    elif "--kernels" in sys.argv:
        kernels(arg("--tag", "kernels"))
    else:
        run(os.path.abspath(arg("--tree", HERE)), arg("--arms", "plain,weighted,masked").split(","), int(arg("--rounds", 5)),
            int(arg("--iters", 10)), arg("--tag", "new"))
