"""The discrete-VAE train step with the EMA codebook ("vq_ema_decay", "vq_restart_after") next to the gradient-trained VQ codebook on
the MI355X, at vae_coco and vae_example and bench.py's batches, on the pattern of tools/vae_vq_bench.py: one model per arm on the same
weights and images in ONE process, rounds alternating which arm runs first; ms per train step (median / min / max over the rounds) and
a SHA-256 of each keys-unset arm's gradients, weights and loss after its first three steps.  --tree DIR imports the model from another
checkout (the parent commit, built there: only the arms plain and vq exist in it), so that a shell loop can alternate this tree and
the parent's; --merge joins the JSON lines of such runs into one file.  The comparison with the parent uses processes of the same
shape on both sides (--arms plain,vq, tags "new" / "parent"); the EMA arms' deltas come from processes holding them next to vq
(tag "pair").
--kernels times, alternating in one process at [16384, 2048, 512] (HIP events around each launch, four buffer sets in rotation):
dmi_vq_cluster_sums against dmi_vq_codebook_grad (the launch it replaces; it accumulates the same sums) with idx uniform and with 90 %
of the rows on one code, dmi_sort_tokens alone on the same idx (what a sorted variant would pay before it adds a row), and
dmi_vq_ema_step against dmi_ema_step over n = T D elements.
Usage: python tools/vae_vq_ema_bench.py [--rounds 5] [--iters 20] [--arms vq,vq_ema,vq_ema_restart] [--models vae_coco,vae_example]
                                        [--tree DIR] [--tag NAME]
       python tools/vae_vq_ema_bench.py --kernels [--tag NAME]
       python tools/vae_vq_ema_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

ARMS = {"plain": {}, "vq": {"quantizer": "vq"}, "vq_ema": {"quantizer": "vq", "vq_ema_decay": 0.99},
        "vq_ema_restart": {"quantizer": "vq", "vq_ema_decay": 0.99, "vq_restart_after": 2}}
KEYS_UNSET = ("plain", "vq")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(tag, M=16384, T=2048, D=512, reps=20, nsets=4):
    """us per launch"""
    for p in (ROOT, os.path.join(ROOT, "dalle-mtf_amd")):
        sys.path.insert(0, p)
    import torch
    import dalle_hip as dh
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    C = (torch.randn(T, D, device=dev, generator=g) * 0.1).bfloat16()
    S = []
    for _ in range(nsets):
        uni = torch.randint(0, T, (M,), device=dev, generator=g, dtype=torch.int32)
        hot = torch.where(torch.rand(M, device=dev, generator=g) < 0.9, torch.full_like(uni, T // 3), uni)
        S.append(dict(x=torch.randn(M, D, device=dev, generator=g).bfloat16(), uniform=uni, skewed=hot, dC=torch.empty(D, T, device=dev),
                      sums=torch.empty(T, D, device=dev), counts=torch.empty(T, dtype=torch.int32, device=dev),
                      c32=torch.randn(D, T, device=dev, generator=g), c16=torch.empty(D, T, dtype=torch.bfloat16, device=dev),
                      N=torch.ones(T, device=dev), S=torch.randn(T, D, device=dev, generator=g),
                      idle=torch.zeros(T, dtype=torch.int32, device=dev), restarts=torch.zeros(1, dtype=torch.int32, device=dev),
                      ema=torch.randn(T * D, device=dev, generator=g), p=torch.randn(T * D, device=dev, generator=g),
                      eb=torch.empty(T * D, dtype=torch.bfloat16, device=dev), st=torch.empty(M, dtype=torch.int32, device=dev),
                      perm=torch.empty(M, dtype=torch.int32, device=dev)))
    ws = torch.empty(int(dh.vq_cluster_sums_workspace_bytes(M, T, D)) + 64, dtype=torch.uint8, device=dev)
    sws = torch.empty(int(dh.sort_tokens_workspace_bytes(M)) + 64, dtype=torch.uint8, device=dev)
    for s in S:      # the EMA step reads the sums of its own set
        dh.vq_cluster_sums(s["x"], D, s["uniform"], s["sums"], s["counts"], M, T, D, ws)
    run = {}
    for kind in ("uniform", "skewed"):
        run["vq_cluster_sums_" + kind] = lambda s, k=kind: dh.vq_cluster_sums(s["x"], D, s[k], s["sums"], s["counts"], M, T, D, ws)
        run["vq_codebook_grad_" + kind] = lambda s, k=kind: dh.vq_codebook_grad(s["x"], D, s[k], C, D, s["dC"], M, T, D)
        run["sort_tokens_" + kind] = lambda s, k=kind: dh.sort_tokens(s[k], s["st"], s["perm"], M, T, sws)
    run["vq_ema_step"] = lambda s: dh.vq_ema_step(s["c32"], s["c16"], s["N"], s["S"], s["idle"], s["restarts"], s["sums"], s["counts"], s["x"], D,
                                                  0.99, 2, 0, 7, M, T, D)
    run["ema_step"] = lambda s: dh.ema_step(s["ema"], s["p"], s["eb"], T * D, 0.01)
    us = {k: [] for k in run}
    for r in range(reps + 3):
        for k in run:
            if k == "vq_ema_step":       # (untimed) the uniform sums again: a skewed launch has overwritten them
                dh.vq_cluster_sums(S[r % nsets]["x"], D, S[r % nsets]["uniform"], S[r % nsets]["sums"], S[r % nsets]["counts"], M, T, D, ws)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run[k](S[r % nsets])
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    med = {k: statistics.median(v) for k, v in us.items()}
    out = dict(tag=tag, shape=[M, T, D], us={k: summary(v) for k, v in us.items()},
               rows_on_the_hot_code=int((S[0]["skewed"] == T // 3).sum()),
               ratios=dict(cluster_sums_over_codebook_grad_uniform=med["vq_cluster_sums_uniform"] / med["vq_codebook_grad_uniform"],
                           cluster_sums_over_codebook_grad_skewed=med["vq_cluster_sums_skewed"] / med["vq_codebook_grad_skewed"],
                           cluster_sums_skewed_over_uniform=med["vq_cluster_sums_skewed"] / med["vq_cluster_sums_uniform"],
                           sort_tokens_alone_over_cluster_sums_uniform=med["sort_tokens_uniform"] / med["vq_cluster_sums_uniform"],
                           vq_ema_step_over_ema_step=med["vq_ema_step"] / med["ema_step"]),
               target="cluster_sums_over_codebook_grad_uniform <= 1.10")
    print(json.dumps(out), flush=True)


def run(tree, arms, models, rounds, iters, tag):
    for p in (tree, os.path.join(tree, "dalle-mtf_amd")):
        sys.path.insert(0, p)
    import torch
    from bench import VAE_MODELS
    from src.vae_tf import DiscreteVAE
    out = {"tag": tag, "models": {}}
    for name in models:
        p = json.load(open(os.path.join(tree, "configs", name + ".json")))
        B = VAE_MODELS[name]
        vaes = {}
        for k in arms:
            vae = DiscreteVAE(num_tokens=p["num_tokens"], dimensions=p["dataset"]["image_size"], convblocks=p["convblocks"],
                              dim=p.get("dim") or 512, hidden_dim=p.get("hidden_dim") or 64, input_channels=p.get("n_channels") or 3,
                              use_bf16=bool(p.get("use_bf16")), recompute_grad=bool(p.get("recompute_grad")),
                              stack_factor=p.get("stack_factor") or 1, batch_size=B, mode="train", **ARMS[k])
            vae.init_params()
            vaes[k] = vae
        g = torch.Generator(device="cuda").manual_seed(1000)
        vae = next(iter(vaes.values()))
        imgs = [(torch.randint(0, 256, (B, vae.H, vae.W, vae.num_ch), device="cuda", generator=g).float() - 127.5) / 127.5 for _ in range(4)]
        noise = [torch.rand(vae.Mg, vae.num_tokens, device="cuda", generator=g).clamp_(1e-9, 0.99999994) for _ in range(3)]
        hard = bool(p.get("train_gumbel_hard", True))
        rec = {"digest_after_3_steps": {}}
        for k in KEYS_UNSET:     # the step without the new keys must compute what the parent commit computes: compare the digests of two trees
            if k in vaes:
                vae = vaes[k]
                for i in range(3):
                    loss = vae.train_step(imgs[i], p["lr"], hard_gumbel=hard, temperature=1.0, noise=noise[i])
                torch.cuda.synchronize()
                h = hashlib.sha256(vae.g.cpu().numpy().tobytes() + vae.p.cpu().numpy().tobytes() + loss.cpu().numpy().tobytes())
                rec["digest_after_3_steps"][k] = h.hexdigest()
        st = {k: [] for k in arms}
        for r in range(rounds):
            for k in (arms if r % 2 == 0 else arms[::-1]):
                vae = vaes[k]
                for i in range(3):
                    vae.train_step(imgs[i % 4], p["lr"], hard_gumbel=hard, temperature=1.0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for i in range(iters):
                    vae.train_step(imgs[i % 4], p["lr"], hard_gumbel=hard, temperature=1.0)
                torch.cuda.synchronize()
                st[k].append((time.perf_counter() - t0) / iters * 1e3)
        rec["step_ms"] = {k: summary(v) for k, v in st.items()}
        rec["batch"] = B
        rec["codebook_stats_after_the_run"] = {k: v.codebook_stats() for k, v in vaes.items() if k != "plain"}
        out["models"][name] = rec
        del vaes
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def merge(path, dest):
    """lines tagged "new" (this tree, keys unset), "parent" (the parent commit, the same arms: the same process shape, so the two compare
    like for like) and "pair" (this tree, the EMA arms next to vq in one process): per-process medians pooled per arm, in the order
    they ran"""
    recs = [json.loads(l) for l in open(path) if l.startswith("{")]
    out = dict(workload="DiscreteVAE.train_step (captured graph), one MI355X, bench.py's batches; per-process medians of alternating "
                        "rounds, three processes per tree alternating in one call", models={})
    for name in sorted({m for r in recs for m in r.get("models", {})}):
        pool, digests, stats = {}, {}, None
        for r in recs:
            m = r.get("models", {}).get(name)
            if m is None:
                continue
            pre = {"parent": "parent_", "pair": "pair_"}.get(r["tag"], "")
            for k, v in m["step_ms"].items():
                pool.setdefault(pre + k, []).append(v["median"])
            for k, d in m.get("digest_after_3_steps", {}).items():
                if r["tag"] in ("new", "parent"):
                    digests.setdefault(k, {}).setdefault(r["tag"], set()).add(d)
            if r["tag"] == "pair":
                stats = m.get("codebook_stats_after_the_run")
        med = lambda k: statistics.median(pool[k])   # noqa: E731
        rec = dict(step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
                   digest_after_3_steps={k: {t: sorted(s) for t, s in v.items()} for k, v in digests.items()})
        for k in ("vq_ema", "vq_ema_restart"):
            if "pair_" + k in pool and "pair_vq" in pool:
                rec[k + "_minus_vq_ms"] = med("pair_" + k) - med("pair_vq")
                rec[k + "_over_vq"] = med("pair_" + k) / med("pair_vq")
        for k in KEYS_UNSET:
            if "parent_" + k in pool and k in pool:
                rec[k + "_minus_parent_ms"] = med(k) - med("parent_" + k)
                rec[k + "_process_spread_ms"] = dict(new=max(pool[k]) - min(pool[k]), parent=max(pool["parent_" + k]) - min(pool["parent_" + k]))
                rec[k + "_per_process_medians_inside_the_parents_range"] = all(
                    min(pool["parent_" + k]) <= v <= max(pool["parent_" + k]) for v in pool[k])
                d = digests.get(k, {})
                rec[k + "_bit_identical_to_parent"] = d.get("new") == d.get("parent") and len(d.get("new", ())) == 1
        if stats:
            rec["codebook_stats_after_the_run"] = stats
        out["models"][name] = rec
    kern = [r for r in recs if "ratios" in r]
    if kern:
        out["kernels"] = kern[-1]
    json.dump(out, open(dest, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    if "--merge" in sys.argv:
        merge(arg("--merge"), arg("--out"))
    elif "--kernels" in sys.argv:
        kernels(arg("--tag", "new"))
    else:
        run(os.path.abspath(arg("--tree", ROOT)), arg("--arms", "vq,vq_ema,vq_ema_restart").split(","),
            arg("--models", "vae_coco,vae_example").split(","), int(arg("--rounds", 5)), int(arg("--iters", 20)), arg("--tag", "new"))
