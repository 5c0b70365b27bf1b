"""The DALL-E train step with and without QK normalisation on the MI355X, at the dalle_example dimensions and bench.py's batch
(B = 32): one engine per arm on the same weights and tokens in ONE process, rounds alternating which arm runs first; ms per train
step (median / min / max over the rounds), a SHA-256 of the plain arm's gradients, weights and loss after its first three steps, and
the kernels alone at the engine's projection buffer ([B S, 3 n_embd] bf16), alternating in the same process: dmi_qk_norm_fwd (with and
without pre) and dmi_qk_norm_bwd, each without a table and fused with the rotation, against dmi_rope_qk (forward and inverse) and
dmi_dropout_bwd over as many elements (the bandwidth yardstick).  Per q / k element dmi_rope_qk and dmi_dropout_bwd move 4 bytes,
dmi_qk_norm_fwd 4 (6 with pre) and dmi_qk_norm_bwd 6 (dqkv in and out, pre in).
--tree DIR imports the engine from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.
Usage: python tools/qk_norm_bench.py [--rounds 5] [--iters 10] [--arms plain,qk,axial,qk_axial] [--tree DIR] [--tag NAME]
       python tools/qk_norm_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

HP = dict(lr=1e-3, train_steps=100000, warmup_steps=3000, gradient_clipping=1.0)
ARMS = {"plain": {}, "qk": {"qk_norm": True}, "axial": {"rotary_emb": "axial"}, "qk_axial": {"qk_norm": True, "rotary_emb": "axial"}}
BYTES = {"rope_qk": 4, "rope_qk_inverse": 4, "dropout_bwd": 4, "qk_norm_fwd_nopre": 4, "qk_norm_fwd": 6, "qk_norm_fwd_rope": 6,
         "qk_norm_bwd": 6, "qk_norm_bwd_rope": 6}        # per q / k element


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
    a, x, pre = (torch.randn(M, 2 * d, device=eng.dev).to(torch.bfloat16) for _ in range(3))
    gq, gk = eng._qk_gains(0)
    dgq, dgk = (torch.empty(hd, dtype=torch.float32, device=eng.dev) for _ in range(2))
    ws = torch.empty(dh.qk_norm_bwd_workspace_bytes(M, hd), dtype=torch.uint8, device=eng.dev)
    cs = eng.rope_cs

    def refill():      # the in-place kernels shrink or grow their operand: every timed launch sees fresh unit-variance values
        qkv.normal_()

    calls = {"rope_qk": lambda: dh.rope_qk(qkv, cs, M, S, H, hd),
             "rope_qk_inverse": lambda: dh.rope_qk(qkv, cs, M, S, H, hd, inverse=True),
             "dropout_bwd": lambda: dh.dropout_bwd(a, x, M, 2 * d, 0x1234567887654321, 6554),
             "qk_norm_fwd_nopre": lambda: dh.qk_norm_fwd(qkv, gq, gk, M, S, H, hd),
             "qk_norm_fwd": lambda: dh.qk_norm_fwd(qkv, gq, gk, M, S, H, hd, pre=pre),
             "qk_norm_fwd_rope": lambda: dh.qk_norm_fwd(qkv, gq, gk, M, S, H, hd, pre=pre, cs=cs),
             "qk_norm_bwd": lambda: dh.qk_norm_bwd(qkv, a, gq, gk, dgq, dgk, ws, M, S, H, hd),
             "qk_norm_bwd_rope": lambda: dh.qk_norm_bwd(qkv, a, gq, gk, dgq, dgk, ws, M, S, H, hd, cs=cs)}
    us = {k: [] for k in calls}
    for r in range(reps + 3):
        for k, f in calls.items():
            refill()
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
        out[k + "_TB_per_s"] = BYTES[k] * M * 2 * d / (out[k]["median"] * 1e-6) / 1e12
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
    if "qk_axial" in engs:
        out["kernels_us"] = kernels(engs["qk_axial"])
        out["pre_bytes"] = sum(t.numel() * t.element_size() for t in engs["qk_axial"].qk_pre)
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
    kmed = {k: statistics.median(r[k]["median"] if isinstance(r[k], dict) else r[k] for r in kern)
            for k in kern[0] if k not in ("shape", "qk_elements")}
    per_byte = {k: kmed[k] / BYTES[k] for k in BYTES}
    fused = dict(forward_fused_us=kmed["qk_norm_fwd_rope"], forward_two_calls_us=kmed["qk_norm_fwd"] + kmed["rope_qk"],
                 backward_fused_us=kmed["qk_norm_bwd_rope"], backward_two_calls_us=kmed["qk_norm_bwd"] + kmed["rope_qk_inverse"])
    fused["fused_not_slower"] = (fused["forward_fused_us"] <= fused["forward_two_calls_us"]
                                 and fused["backward_fused_us"] <= fused["backward_two_calls_us"])
    out = dict(workload="dalle_example train step, B = 32, one MI355X; per-process medians of alternating rounds, processes of the "
                        "two trees alternating in one call; qk = qk_norm (6 dmi_qk_norm_fwd + 6 dmi_qk_norm_bwd launches per step), "
                        "axial = rotary_emb 'axial' (6 + 6 dmi_rope_qk launches), qk_axial = both (the fused launches)",
               step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
               qk_minus_plain_ms=med("qk") - med("plain"), qk_over_plain=med("qk") / med("plain"),
               qk_axial_minus_axial_ms=med("qk_axial") - med("axial"), qk_axial_minus_plain_ms=med("qk_axial") - med("plain"),
               plain_minus_parent_ms=diff, process_spread_ms=spread,
               plain_minus_parent_inside_spread=abs(diff) <= max(spread.values()),
               plain_digest_after_3_steps=digests,
               key_unset_bit_identical_to_parent=len({d for v in digests.values() for d in v}) == 1 and len(digests) == 2,
               pre_bytes=next((r["pre_bytes"] for r in recs if "pre_bytes" in r), None),
               kernels_us=dict(median_over_processes=kmed, bytes_per_qk_element=BYTES, us_per_byte_per_element=per_byte,
                               per_byte_over_rope_qk={k: per_byte[k] / per_byte["rope_qk"] for k in BYTES if k.startswith("qk_norm")},
                               per_byte_over_dropout_bwd={k: per_byte[k] / per_byte["dropout_bwd"] for k in BYTES if k.startswith("qk_norm")},
                               streaming_target=1.10, fused_against_two_calls=fused, per_process=kern, shape=kern[0]["shape"],
                               qk_elements=kern[0]["qk_elements"]))
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    else:
        run(os.path.abspath(arg("--tree", os.path.dirname(os.path.dirname(os.path.abspath(__file__))))),
            arg("--arms", "plain,qk,axial,qk_axial").split(","), int(arg("--rounds", 5)), int(arg("--iters", 10)), arg("--tag", "new"))
