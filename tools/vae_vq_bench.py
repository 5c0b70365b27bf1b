"""The discrete-VAE train step with the Gumbel and with the vector-quantised bottleneck on the MI355X, at vae_coco and vae_example and
bench.py's batches (16 / 32): one model per arm on the same weights and images in ONE process, rounds alternating which arm runs
first; ms per train step (median / min / max over the rounds) and a SHA-256 of the plain arm's gradients, weights and loss after its
first three steps.  --tree DIR imports the model from another checkout (the parent commit, built there: only --arms plain exists in
it), so that a shell loop can alternate this tree and the parent's; --merge joins the JSON lines of such runs into one file.  The
comparison with the parent uses processes of the same shape on both sides (--arms plain, tags "new" / "parent"); the VQ arm's delta
comes from processes holding both arms (tag "pair").
--kernels times dmi_vq_assign alone at [16384, 2048, 512] against the dmi_gemm_nt(..., OUT_F32) logits product of the same shape, and
dmi_vq_loss, dmi_vq_bwd_x and dmi_vq_codebook_grad per byte moved against dmi_gumbel_softmax_bwd at [16384, 2048], all in one process
(bytes from the shapes; four buffer sets in rotation; HIP events around each launch, the kernels alternating).
Usage: python tools/vae_vq_bench.py [--rounds 5] [--iters 20] [--arms plain,vq] [--models vae_coco,vae_example] [--tree DIR] [--tag NAME]
       python tools/vae_vq_bench.py --kernels [--tag NAME]
       python tools/vae_vq_bench.py --merge LINES.jsonl --out FILE"""
import hashlib
import json
import os
import statistics
import sys
import time

ARMS = {"plain": {}, "vq": {"quantizer": "vq"}}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def summary(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs), n=len(xs))


def kernels(tag, M=16384, T=2048, D=512, reps=20, nsets=4):
    """us per launch.  Bytes from the shapes: assign reads X and the codebook once per 64-row block from L2 (HBM: 2 M D + 2 T D),
    writes idx and xq; the logits product reads the same and writes 4 M T; vq_loss 2 + 2 read per element of [M, D]; vq_bwd_x
    2 + 2 + 2 read, 2 written; vq_codebook_grad X, idx and the codebook read, the [D, T] fp32 gradient written; gumbel_bwd 2 + 2 read,
    2 written per element of [M, T]"""
    for p in (ROOT, os.path.join(ROOT, "dalle-mtf_amd")):
        sys.path.insert(0, p)
    import torch
    import dalle_hip as dh
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(1)
    C = (torch.randn(T, D, device=dev, generator=g) * 0.1).bfloat16()
    h = torch.empty(T, device=dev)
    dh.vq_half_norms(h, T, D, codebook_t=C, ldc=D)
    S = []
    for _ in range(nsets):
        code = torch.randint(0, T, (M,), device=dev, generator=g)
        x = (C[code].float() + 0.05 * torch.randn(M, D, device=dev, generator=g)).bfloat16()       # the trained regime: near a code
        S.append(dict(x=x, idx=torch.empty(M, dtype=torch.int32, device=dev), xq=torch.empty(M, D, dtype=torch.bfloat16, device=dev),
                      logits=torch.empty(M, T, device=dev), d=(torch.randn(M, D, device=dev, generator=g) * 1e-4).bfloat16(),
                      dx=torch.empty(M, D, dtype=torch.bfloat16, device=dev), dC=torch.empty(D, T, device=dev),
                      dy=(torch.randn(M, T, device=dev, generator=g) * 0.01).bfloat16(),
                      ys=torch.rand(M, T, device=dev, generator=g).bfloat16(), dl=torch.empty(M, T, dtype=torch.bfloat16, device=dev)))
    for s in S:
        dh.vq_assign(s["x"], D, C, D, h, s["idx"], s["xq"], D, None, M, T, D)
    lq = torch.zeros(1, device=dev)
    ws = torch.empty(int(dh.vq_loss_workspace_bytes()) + 64, dtype=torch.uint8, device=dev)
    nbytes = dict(vq_assign=2.0 * M * D + 2.0 * T * D + 4.0 * M + 2.0 * M * D, logits_gemm=2.0 * M * D + 2.0 * T * D + 4.0 * M * T,
                  vq_loss=4.0 * M * D, vq_bwd_x=8.0 * M * D, vq_codebook_grad=2.0 * M * D + 4.0 * M + 2.0 * T * D + 4.0 * T * D,
                  gumbel_bwd=6.0 * M * T)
    run = dict(vq_assign=lambda s: dh.vq_assign(s["x"], D, C, D, h, s["idx"], s["xq"], D, None, M, T, D),
               logits_gemm=lambda s: dh.gemm_nt(s["x"], D, C, D, s["logits"], T, M, T, D, dh.GEMM_OUT_F32),
               vq_loss=lambda s: dh.vq_loss(s["x"], D, s["xq"], D, lq, M, D, ws),
               vq_bwd_x=lambda s: dh.vq_bwd_x(s["d"], D, s["x"], D, s["xq"], D, s["dx"], D, M, D, 0.25),
               vq_codebook_grad=lambda s: dh.vq_codebook_grad(s["x"], D, s["idx"], C, D, s["dC"], M, T, D),
               gumbel_bwd=lambda s: dh.gumbel_softmax_bwd(s["dy"], s["ys"], s["dl"], M, T, 1.0))
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
    out = dict(tag=tag, shape=[M, T, D], us={k: summary(v) for k, v in us.items()}, bytes=nbytes,
               codes_used=int(torch.unique(S[0]["idx"]).numel()))
    med = {k: out["us"][k]["median"] for k in run}
    out["TB_per_s"] = {k: nbytes[k] / (med[k] * 1e-6) / 1e12 for k in run}
    out["TFLOP_per_s"] = {k: 2.0 * M * T * D / (med[k] * 1e-6) / 1e12 for k in ("vq_assign", "logits_gemm")}
    tb = out["TB_per_s"]
    # > 1 = slower than the neighbour: assign in time against the product; the streaming kernels in time per byte against gumbel_bwd
    out["vs_neighbour"] = dict(vq_assign_vs_logits_gemm_time=med["vq_assign"] / med["logits_gemm"],
                               vq_loss_vs_gumbel_bwd_per_byte=tb["gumbel_bwd"] / tb["vq_loss"],
                               vq_bwd_x_vs_gumbel_bwd_per_byte=tb["gumbel_bwd"] / tb["vq_bwd_x"],
                               vq_codebook_grad_vs_gumbel_bwd_per_byte=tb["gumbel_bwd"] / tb["vq_codebook_grad"])
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
        if "vq" in vaes:
            rec["vq_codes_used_frac_after_the_run"] = vaes["vq"].codebook_stats()["codes_used_frac"]
        out["models"][name] = rec
        del vaes
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def merge(path, dest):
    """lines tagged "new" (this tree, plain arm alone), "parent" (the parent commit, plain arm alone: the same process shape, so the
    two compare like for like) and "pair" (this tree, both arms in one process: the VQ arm next to the Gumbel arm): per-process medians
    pooled per arm, in the order they ran"""
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
            if m.get("plain_digest_after_3_steps"):
                digests.setdefault("parent" if r["tag"] == "parent" else "new", set()).add(m["plain_digest_after_3_steps"])
        med = lambda k: statistics.median(pool[k])   # noqa: E731
        rec = dict(step_ms={k: dict(summary(v), per_process_medians=v) for k, v in pool.items()},
                   plain_digest_after_3_steps={k: sorted(v) for k, v in digests.items()})
        if "pair_vq" in pool and "pair_plain" in pool:
            rec["vq_minus_plain_ms"] = med("pair_vq") - med("pair_plain")
            rec["vq_over_plain"] = med("pair_vq") / med("pair_plain")
        if "parent_plain" in pool and "plain" in pool:
            rec["plain_minus_parent_ms"] = med("plain") - med("parent_plain")
            rec["process_spread_ms"] = dict(plain=max(pool["plain"]) - min(pool["plain"]),
                                            parent_plain=max(pool["parent_plain"]) - min(pool["parent_plain"]))
            rec["key_unset_bit_identical_to_parent"] = digests.get("new") == digests.get("parent") and len(digests["new"]) == 1
        out["models"][name] = rec
    kern = [r for r in recs if "vs_neighbour" in r]
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
        run(os.path.abspath(arg("--tree", ROOT)), arg("--arms", "plain,vq").split(","), arg("--models", "vae_coco,vae_example").split(","),
            int(arg("--rounds", 5)), int(arg("--iters", 20)), arg("--tag", "new"))
