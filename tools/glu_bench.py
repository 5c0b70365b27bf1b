"""The DALL-E train step with and without the gated feed-forward on the MI355X, at the dalle_example dimensions and bench.py's batch
(B = 32): one engine per arm on the same tokens in ONE process, rounds alternating which arm runs first; ms per train step (median /
min / max over the rounds), a SHA-256 of the plain arm's gradients, weights and loss after its first three steps, and dmi_glu_fwd /
dmi_glu_bwd alone at [B S, 4 n_embd], alternating with dmi_dropout_bwd over buffers of the same total bytes (it streams 2 B in and
2 B out per element: the bandwidth yardstick; the target is 1.10 x its time per byte moved).
Arms: plain (the key unset, ReLU -- what the parent commit runs), gelu (activation_fn gelu, the key unset), geglu (both).
--tree DIR imports the engine from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.
Usage: python tools/glu_bench.py [--rounds 6] [--iters 20] [--arms plain,gelu,geglu] [--tree DIR] [--tag NAME]
       python tools/glu_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
ARMS = {"plain": {}, "gelu": {"activation_fn": "gelu"}, "geglu": {"activation_fn": "gelu", "ff_glu": True}}


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(M, Hh, reps=30):
    """us per launch, HIP events around each launch, the kernels alternating.  Bytes moved: glu_fwd 6 M Hh (pre in, h out), glu_bwd
    10 M Hh (dh and pre in, dpre out); dropout_bwd runs over [M, 1.5 Hh] and [M, 2.5 Hh] elements: the same totals"""
    import torch
    import dalle_hip as dh
    dev = "cuda"
    pre = (torch.randn(M, 2 * Hh, device=dev) * 3).to(torch.bfloat16)
    dhh = torch.randn(M, Hh, device=dev).to(torch.bfloat16)
    h = torch.empty(M, Hh, dtype=torch.bfloat16, device=dev)
    dpre = torch.empty(M, 2 * Hh, dtype=torch.bfloat16, device=dev)
    xa, ya = (torch.randn(M, 3 * Hh // 2, device=dev).to(torch.bfloat16) for _ in range(2))
    xb, yb = (torch.randn(M, 5 * Hh // 2, device=dev).to(torch.bfloat16) for _ in range(2))
    key, th = 0x1234567887654321, 6554
    calls = {"glu_fwd_gelu": lambda: dh.glu_fwd(pre, 2 * Hh, h, Hh, M, Hh, "gelu"),
             "glu_fwd_relu": lambda: dh.glu_fwd(pre, 2 * Hh, h, Hh, M, Hh, "relu"),
             "dropout_bwd_fwd_bytes": lambda: dh.dropout_bwd(xa, ya, M, 3 * Hh // 2, key, th),
             "glu_bwd_gelu": lambda: dh.glu_bwd(dhh, Hh, pre, 2 * Hh, dpre, 2 * Hh, M, Hh, "gelu"),
             "glu_bwd_relu": lambda: dh.glu_bwd(dhh, Hh, pre, 2 * Hh, dpre, 2 * Hh, M, Hh, "relu"),
             "dropout_bwd_bwd_bytes": lambda: dh.dropout_bwd(xb, yb, M, 5 * Hh // 2, key, th)}
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
    out["shape"] = [M, Hh]
    nbytes = {"glu_fwd": 6 * M * Hh, "glu_bwd": 10 * M * Hh}
    for k in ("glu_fwd_gelu", "glu_fwd_relu", "glu_bwd_gelu", "glu_bwd_relu"):
        yard = "dropout_bwd_fwd_bytes" if "fwd" in k else "dropout_bwd_bwd_bytes"
        out[k + "_TB_per_s"] = nbytes[k[:7]] / (out[k]["median"] * 1e-6) / 1e12
        out[k + "_over_dropout_bwd_same_bytes"] = out[k]["median"] / out[yard]["median"]
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
    if "geglu" in engs:
        e = engs["geglu"]
        out["geglu_forms"] = dict(ffn_form=e.ffn_form, fuse_ln=bool(e.fuse_ln), fuse_lnbwd=bool(e.fuse_lnbwd), wgrad_group4=bool(e.wgrad_group4),
                                  parameters=int(e.lay.total))
        M, Hh = e.M, 4 * e.d
        del engs, eng, e
        torch.cuda.empty_cache()
        out["kernels_us"] = kernels(M, Hh)
    print(json.dumps(out), flush=True)


def merge(path, dest):
    """lines tagged "new" (every arm) and "parent" (plain): pooled per arm, in the order they ran"""
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
    spread = dict(plain=max(pool["plain"]) - min(pool["plain"]), parent_plain=max(pool["parent_plain"]) - min(pool["parent_plain"]))
    diff = med("plain") - med("parent_plain")
    out = dict(workload="dalle_example train step, B = 32, one MI355X; per-process medians of alternating rounds, processes of the two "
                        "trees alternating in one call; plain = the key unset (ReLU), gelu = activation_fn gelu, geglu = gelu + ff_glu "
                        "(mlp_linear_1 [d, 8d]: 4 d^2 + 4 d more parameters per layer, one dmi_glu_fwd and one dmi_glu_bwd per block)",
               step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
               plain_minus_parent_ms=diff, process_spread_ms=spread,
               plain_minus_parent_inside_parent_spread=abs(diff) <= spread["parent_plain"],
               plain_digest_after_3_steps=digests,
               key_unset_bit_identical_to_parent=len({d for v in digests.values() for d in v}) == 1 and len(digests) == 2)
    if "geglu" in pool and "gelu" in pool:
        out.update(geglu_minus_gelu_ms=med("geglu") - med("gelu"), geglu_over_gelu=med("geglu") / med("gelu"),
                   geglu_forms=next(r["geglu_forms"] for r in recs if "geglu_forms" in r))
    if kern:
        kmed = {k: statistics.median(r[k]["median"] if isinstance(r[k], dict) else r[k] for r in kern) for k in kern[0] if k != "shape"}
        ratios = {k: v for k, v in kmed.items() if k.endswith("_over_dropout_bwd_same_bytes")}
        out["kernels_us"] = dict(median_over_processes=kmed, per_process=kern, shape=kern[0]["shape"],
                                 target="each glu kernel within 1.10 x dmi_dropout_bwd over the same total bytes",
                                 within_target={k: v <= 1.10 for k, v in ratios.items()})
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    else:
        run(os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            arg("--arms", "plain,gelu,geglu").split(","), int(arg("--rounds", 6)), int(arg("--iters", 20)), arg("--tag", "new"))
