"""The DALL-E train step with and without token shift on the MI355X, at the dalle_example dimensions and bench.py's batch (B = 32):
one engine per arm on the same weights and tokens in ONE process, rounds alternating which arm runs first; ms per train step
(median / min / max over the rounds), a SHA-256 of the plain arm's gradients, weights and loss after its first three steps, and
dmi_token_shift alone over the engine's [B S, n_embd] bf16 rows, forward and inverse, alternating with dmi_dropout_bwd over the
same two buffers (it reads and writes the same bytes: the bandwidth yardstick; the target is 1.10 x its median).
--tree DIR imports the engine from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.
Usage: python tools/token_shift_bench.py [--rounds 5] [--iters 10] [--arms plain,shift] [--tree DIR] [--tag NAME]
       python tools/token_shift_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
ARMS = {"plain": {}, "shift": {"token_shift": True}}


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(eng, reps=30):
    """us per launch at the engine's shapes, HIP events around each launch, the kernels alternating"""
    import torch
    import dalle_hip as dh
    M, d, S, T, G = eng.M, eng.d, eng.S, eng.T, eng.G
    x, y = (torch.randn(M, d, device=eng.dev).to(torch.bfloat16) for _ in range(2))
    calls = {"token_shift": lambda: dh.token_shift(x, y, M, S, T, G, d),
             "token_shift_inverse": lambda: dh.token_shift(x, y, M, S, T, G, d, inverse=True),
             "dropout_bwd": lambda: dh.dropout_bwd(x, y, M, d, 0x1234567887654321, 6554)}
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
    out["shape"] = [M, d]
    for k in calls:                      # 2 B read + 2 B written per element (the zeroed pieces are written, not read)
        out[k + "_TB_per_s"] = 4 * M * d / (out[k]["median"] * 1e-6) / 1e12
    for k in ("token_shift", "token_shift_inverse"):
        out[k + "_over_dropout_bwd"] = out[k]["median"] / out["dropout_bwd"]["median"]
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
    on = [k for k in arms if k != "plain"]
    if on:
        out["kernels_us"] = kernels(engs[on[0]])
    print(json.dumps(out), flush=True)


def merge(path, dest):
    """lines tagged "new" (the plain and the shift arm) and "parent" (plain): pooled per arm, in the order they ran"""
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
    on = next(k for k in pool if k not in ("plain", "parent_plain"))
    spread = dict(plain=max(pool["plain"]) - min(pool["plain"]), parent_plain=max(pool["parent_plain"]) - min(pool["parent_plain"]))
    diff = med("plain") - med("parent_plain")
    kmed = {k: statistics.median(r[k]["median"] if isinstance(r[k], dict) else r[k] for r in kern)
            for k in kern[0] if k != "shape"}
    out = dict(workload="dalle_example train step, B = 32, one MI355X; per-process medians of alternating rounds, processes of the "
                        f"two trees alternating in one call; {on} = token_shift true (2 dmi_token_shift launches per block in the "
                        "forward, 2 inverse ones in the backward, and the unfused LayerNorm backward)",
               step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
               shift_minus_plain_ms=med(on) - med("plain"), shift_over_plain=med(on) / med("plain"),
               plain_minus_parent_ms=diff, process_spread_ms=spread,
               plain_minus_parent_inside_spread=abs(diff) <= max(spread.values()),
               plain_digest_after_3_steps=digests,
               key_unset_bit_identical_to_parent=len({d for v in digests.values() for d in v}) == 1 and len(digests) == 2,
               kernels_us=dict(median_over_processes=kmed, per_process=kern, shape=kern[0]["shape"],
                               target="token_shift and token_shift_inverse within 1.10 x dropout_bwd",
                               within_target=max(kmed["token_shift"], kmed["token_shift_inverse"]) <= 1.10 * kmed["dropout_bwd"]))
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    else:
        run(os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            arg("--arms", "plain,shift").split(","), int(arg("--rounds", 5)), int(arg("--iters", 10)), arg("--tag", "new"))
