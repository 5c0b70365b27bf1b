"""The DALL-E train step with and without embedding / residual dropout on the MI355X, at the dalle_example dimensions and bench.py's
batch (B = 32): one engine per arm on the same weights and tokens in ONE process, rounds alternating which arm runs first; ms per
train step (median / min / max over the rounds), a SHA-256 of the plain arm's gradients, weights and loss after its first three
steps, and the dropout kernels alone at the engine's shapes ([B S, n_embd] bf16): dmi_dropout_add_ln (8 B per element: a and the
residual in, x and the LayerNorm out), dmi_dropout_bwd (4 B), dmi_embed_fwd_dropout, beside dmi_layernorm_fwd (4 B) for scale.
--tree DIR imports the engine from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.
Usage: python tools/dropout_bench.py [--rounds 5] [--iters 10] [--arms plain,drop] [--tree DIR] [--tag NAME]
       python tools/dropout_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
ARMS = {"plain": {}, "drop": {"residual_dropout": 0.1, "embed_dropout": 0.1}}


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(eng, reps=30):
    """us per launch at the engine's shapes, HIP events around each launch, the kernels alternating"""
    import torch
    import dalle_hip as dh
    M, d, S = eng.M, eng.d, eng.S
    a, res, x, y = (torch.randn(M, d, device=eng.dev).to(torch.bfloat16) for _ in range(4))
    mean, rstd = torch.empty(M, device=eng.dev), torch.empty(M, device=eng.dev)
    g, b = eng._w("layer_0/norm_2/g"), eng._w("layer_0/norm_2/b")
    wte, wpe = eng._w("embedding/wte"), eng._w("positional_embedding/wpe")
    key, thresh = 0x1234567887654321, eng.resid_thresh
    calls = {"dropout_add_ln": lambda: dh.dropout_add_ln(a, res, x, g, b, y, mean, rstd, M, d, key, thresh),
             "dropout_bwd": lambda: dh.dropout_bwd(a, x, M, d, key, thresh),
             "embed_fwd_dropout": lambda: dh.embed_fwd_dropout(eng.tokens, wte, wpe, x, S, d, eng.V, key, key + 1, eng.embed_thresh),
             "layernorm_fwd": lambda: dh.layernorm_fwd(res, g, b, y, mean, rstd, M, d),
             "embed_fwd": lambda: dh.embed_fwd(eng.tokens, wte, wpe, x, S, d, eng.V)}
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
    out["elements"] = M * d
    for k, nbytes in (("dropout_add_ln", 8), ("dropout_bwd", 4), ("layernorm_fwd", 4)):
        out[k + "_TB_per_s"] = nbytes * M * d / (out[k]["median"] * 1e-6) / 1e12
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
    if "plain" in engs:      # the step without the keys must compute what the parent commit computes: compare the digests of two trees
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
    if "drop" in engs:
        out["kernels_us"] = kernels(engs["drop"])
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
    spread = dict(plain=max(pool["plain"]) - min(pool["plain"]), parent_plain=max(pool["parent_plain"]) - min(pool["parent_plain"]))
    diff = med("plain") - med("parent_plain")
    kmed = {k: statistics.median(r[k]["median"] if isinstance(r[k], dict) else r[k] for r in kern) for k in kern[0] if k != "elements"}
    out = dict(workload="dalle_example train step, B = 32, one MI355X; per-process medians of alternating rounds, processes of the "
                        "two trees alternating in one call; drop = residual_dropout 0.1 + embed_dropout 0.1",
               step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
               drop_minus_plain_ms=med("drop") - med("plain"), drop_over_plain=med("drop") / med("plain"),
               plain_minus_parent_ms=diff, process_spread_ms=spread,
               plain_minus_parent_inside_spread=abs(diff) <= max(spread.values()),
               plain_digest_after_3_steps=digests, keys_unset_bit_identical_to_parent=digests.get("new") == digests.get("parent"),
               kernels_us=dict(median_over_processes=kmed, per_process=kern, elements=kern[0]["elements"]))
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    else:
        run(os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            arg("--arms", "plain,drop").split(","), int(arg("--rounds", 5)), int(arg("--iters", 10)), arg("--tag", "new"))
