"""The discrete-VAE train step with and without the KL term on the MI355X, at vae_coco and vae_example and bench.py's batches (16 / 32):
one model per arm on the same weights and images in ONE process, rounds alternating which arm runs first; ms per train step
(median / min / max over the rounds) and a SHA-256 of the plain arm's gradients, weights and loss after its first three steps.
--tree DIR imports the model from another checkout (the parent commit, built there: only --arms plain exists in it), so that a
shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.  The comparison with
the parent uses processes of the same shape on both sides (--arms plain, tags "new" / "parent": one model per process, so that
the two trees are measured like for like); the KL term's delta comes from processes holding both arms (tag "pair").
--kernels times the three new kernels alone at [16384, 2048] against dmi_gumbel_softmax_fwd / _bwd in the same process, per byte
moved (bytes from the shapes; four buffer sets in rotation, 0.5 GiB of logits, so that no launch finds its input in a cache).
Usage: python tools/vae_kl_bench.py [--rounds 5] [--iters 20] [--arms plain,kl] [--models vae_coco,vae_example] [--tree DIR] [--tag NAME]
       python tools/vae_kl_bench.py --kernels [--tag NAME]
       python tools/vae_kl_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

ARMS = {"plain": {}, "kl": {"kl_loss_weight": 1.0}}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(tag, M=16384, T=2048, reps=20, nsets=4):
    """us per launch, HIP events around each launch, the five kernels alternating; bytes per element from the shapes:
    gumbel_fwd 4 + 4 read, 2 + 2 written; gumbel_bwd 2 + 2 read, 2 written; kl_fwd 4 read; bwd_kl 2 + 2 + 4 read, 2 written;
    usage 4 read (+ its [slabs][T] partials, written and read once)"""
    for p in (ROOT, os.path.join(ROOT, "dalle-mtf_amd")):
        sys.path.insert(0, p)
    import torch
    import dalle_hip as dh
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    S = []
    for _ in range(nsets):
        l = torch.randn(M, T, device=dev, generator=g) * 2
        S.append(dict(l=l, u=torch.rand(M, T, device=dev, generator=g).clamp_(1e-9, 0.99999994),
                      y=torch.empty(M, T, dtype=torch.bfloat16, device=dev), ys=torch.empty(M, T, dtype=torch.bfloat16, device=dev),
                      idx=torch.empty(M, dtype=torch.int32, device=dev), dy=(torch.randn(M, T, device=dev, generator=g) * 0.01).bfloat16(),
                      dl=torch.empty(M, T, dtype=torch.bfloat16, device=dev), rs=torch.empty(M, 2, device=dev)))
    kl, qsum, counts = torch.zeros(1, device=dev), torch.empty(T, device=dev), torch.empty(T, dtype=torch.int32, device=dev)
    ws = torch.empty(int(dh.codebook_kl_workspace_bytes(M, T)) + 64, dtype=torch.uint8, device=dev)
    slabs = min((M + 31) // 32, 512)
    per_elt = dict(gumbel_fwd=12.0, gumbel_bwd=6.0, kl_fwd=4.0, bwd_kl=10.0, usage=4.0 + 2.0 * 8.0 * slabs / M)
    run = dict(gumbel_fwd=lambda s: dh.gumbel_softmax_fwd(s["l"], s["u"], s["y"], s["ys"], s["idx"], M, T, 1.0, True),
               gumbel_bwd=lambda s: dh.gumbel_softmax_bwd(s["dy"], s["ys"], s["dl"], M, T, 1.0),
               kl_fwd=lambda s: dh.codebook_kl_fwd(s["l"], s["rs"], kl, M, T, ws),
               bwd_kl=lambda s: dh.gumbel_softmax_bwd_kl(s["dy"], s["ys"], s["l"], s["rs"], s["dl"], M, T, 1.0, 1.0),
               usage=lambda s: dh.codebook_usage(s["l"], s["rs"], s["idx"], qsum, counts, M, T, ws))
    us = {k: [] for k in run}
    for r in range(reps + 3):
        for k, fn in run.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn(S[r % nsets])
            e1.record()
            torch.cuda.synchronize()
            if r >= 3:
                us[k].append(e0.elapsed_time(e1) * 1e3)
    out = dict(tag=tag, shape=[M, T], us={k: summary(v) for k, v in us.items()}, bytes_per_element=per_elt)
    out["TB_per_s"] = {k: per_elt[k] * M * T / (out["us"][k]["median"] * 1e-6) / 1e12 for k in run}
    tb = out["TB_per_s"]
    # time per byte against the neighbour: > 1 = slower per byte than the neighbour
    out["per_byte_vs_neighbour"] = dict(kl_fwd_vs_gumbel_fwd=tb["gumbel_fwd"] / tb["kl_fwd"], usage_vs_gumbel_fwd=tb["gumbel_fwd"] / tb["usage"],
                                        bwd_kl_vs_gumbel_bwd=tb["gumbel_bwd"] / tb["bwd_kl"])
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
        rec = {}
        if "plain" in vaes:      # the step without the key must compute what the parent commit computes: compare the digests of two trees
            vae = vaes["plain"]
            for i in range(3):
                loss = vae.train_step(imgs[i], p["lr"], hard_gumbel=hard, temperature=1.0, noise=noise[i])
            torch.cuda.synchronize()
            h = hashlib.sha256(vae.g.cpu().numpy().tobytes() + vae.p.cpu().numpy().tobytes() + loss.cpu().numpy().tobytes())
            rec["plain_digest_after_3_steps"] = h.hexdigest()
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
        out["models"][name] = rec
        del vaes
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def merge(path, dest):
    """lines tagged "new" (this tree, plain arm alone), "parent" (the parent commit, plain arm alone: the same process shape, so the
    two compare like for like) and "pair" (this tree, both arms in one process: the KL term's delta): per-process medians pooled per
    arm, in the order they ran"""
    recs = [json.loads(l) for l in open(path) if l.startswith("{")]
    out = dict(workload="DiscreteVAE.train_step (captured graph), one MI355X, bench.py's batches; per-process medians of alternating "
                        "rounds, three processes per tree alternating in one call", models={})
    for name in sorted({m for r in recs for m in r.get("models", {})}):
        pool, digests = {}, {}
        for r in recs:
            m = r.get("models", {}).get(name)
            if m is None:
                continue
            for k, v in m["step_ms"].items():
                pool.setdefault({"parent": "parent_", "pair": "pair_"}.get(r["tag"], "") + k, []).append(v["median"])
            digests.setdefault("parent" if r["tag"] == "parent" else "new", set()).add(m.get("plain_digest_after_3_steps"))
        med = lambda k: statistics.median(pool[k])   # noqa: E731
        rec = dict(step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
                   plain_digest_after_3_steps={k: sorted(v) for k, v in digests.items()})
        if "pair_kl" in pool and "pair_plain" in pool:
            rec["kl_minus_plain_ms"] = med("pair_kl") - med("pair_plain")
        if "parent_plain" in pool and "plain" in pool:
            rec["plain_minus_parent_ms"] = med("plain") - med("parent_plain")
            rec["process_spread_ms"] = dict(plain=max(pool["plain"]) - min(pool["plain"]),
                                            parent_plain=max(pool["parent_plain"]) - min(pool["parent_plain"]))
            rec["keys_unset_bit_identical_to_parent"] = digests.get("new") == digests.get("parent") and len(digests["new"]) == 1
        out["models"][name] = rec
    kern = [r for r in recs if "per_byte_vs_neighbour" in r]
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
        run(os.path.abspath(arg("--tree", ROOT)), arg("--arms", "plain,kl").split(","), arg("--models", "vae_coco,vae_example").split(","),
            int(arg("--rounds", 5)), int(arg("--iters", 20)), arg("--tag", "new"))
