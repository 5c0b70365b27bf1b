"""Generation throughput in one process (random weights): the KV-cached graph sampler against the plain sampler (one full
forward per position), and the per-position cost of the draw variants (top-k, top-k + top-p, + log-likelihood).
    python tools/genbench.py --shape example|coco --batch B [--kv-cache-dtype bf16|fp8|both] [--guidance-scale S] [--rotary 1d|axial] [--token-shift] [--ff-glu] [--qk-norm] [--activation relu|gelu] [--out FILE.json]
    python tools/genbench.py --kernels        # the two draw kernels alone (time them under rocprofv3 --kernel-trace --stats)
The plain sampler is timed over its last --plain-positions positions (an image prefix teacher-forces the rest; each of its
positions is one full forward, so the rate does not depend on which positions are timed).
--guidance-scale S != 1 times the guided sampler instead: the engine's B rows are B / 2 (caption, null caption) pairs, rates count
the B / 2 generated rows, and the plain sampler is left out.
--rotary SCHEME sets the config key "rotary_emb": one dmi_rope_qk_decode launch more per layer and position.
--token-shift sets the config key "token_shift": the two block LayerNorms of every layer leave the fused prologue form, and one
dmi_token_shift_decode launch follows each.
--ff-glu sets the config key "ff_glu" (with --activation gelu: GEGLU): FFN-1 of the decode step is 8 n_embd wide with its bias only, and
one dmi_glu_fwd launch follows it.
--qk-norm sets the config key "qk_norm": one dmi_qk_norm_decode launch more per layer and position (with --rotary it takes the place
of dmi_rope_qk_decode).
--kv-cache-dtype fp8 times the sampler on the FP8 key/value cache; both: bf16 and fp8 alternating in one process (rounds of one timed
call each, the median reported per type under "bf16" / "fp8", with the cache bytes and a hash of the sampled tokens), nothing else."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
import torch  # noqa: E402

SHAPES = {"example": dict(d=512, L=6, H=4, iv=512, hp={}),                        # configs/dalle_example.json
          "coco": dict(d=1024, L=12, H=8, iv=2048, hp=dict(recompute_grad=True))}  # configs/dalle_coco.json (recompute on)


def timed(fn, reps=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps, r


# command-line option -> (the argparse arguments of its flag, the config key it sets); the keys that are set also go into the result
OPTIONS = {"rotary": (dict(choices=("1d", "axial"), default=None), "rotary_emb"),
           "token_shift": (dict(action="store_true"), "token_shift"),
           "ff_glu": (dict(action="store_true"), "ff_glu"),
           "qk_norm": (dict(action="store_true"), "qk_norm"),
           "activation": (dict(choices=("relu", "gelu"), default=None), "activation_fn")}


def engine_bench(shape, B, plain_positions, guidance_scale=1.0, kv_cache_dtype=None, **options):
    """options: the values of OPTIONS' command-line options; one that is unset or false sets no key"""
    from src.dalle_mtf.engine import DalleEngine
    c = SHAPES[shape]
    T, P, tv = 256, 1024, 50258
    keys = {OPTIONS[name][1]: value for name, value in options.items() if value}
    eng = DalleEngine(c["d"], c["L"], c["H"], tv, c["iv"], T, P, batch_size=B, hparams=dict(lr=1e-3, train_steps=10, **c["hp"], **keys))
    eng.init_params(seed=1)
    guided = guidance_scale != 1.0
    R = B // 2 if guided else B                   # generated rows per call
    gkw = dict(guidance_scale=guidance_scale) if guided else {}
    text = torch.randint(0, tv - 1, (R, T), dtype=torch.int32, device="cuda")
    res = dict(shape=shape, batch=B, guidance_scale=guidance_scale, rows_generated=R, n_embd=c["d"], n_layers=c["L"], n_heads=c["H"], seq=T + P, image_vocab=c["iv"],
               recompute_grad=bool(eng.recompute), **keys)
    if kv_cache_dtype == "both":
        return dict(res, **kv_pair_bench(eng, text, R, P, c, B, T + P, gkw))
    if kv_cache_dtype is not None:
        res["kv_cache_dtype"] = kv_cache_dtype
        gkw["kv_cache_dtype"] = kv_cache_dtype
    variants = (("top_k", dict(temperature=1.0, top_k=32)), ("top_k+top_p", dict(temperature=1.0, top_k=32, top_p=0.9)),
                ("top_k+top_p+logp", dict(temperature=1.0, top_k=32, top_p=0.9, return_logprobs=True)),
                ("top_p", dict(temperature=1.0, top_p=0.9)))
    for _, kw in variants:
        eng.sample_image_tokens(text, seed=0, **kw, **gkw)        # warm-up: caches, graph capture per variant
        eng.sample_image_tokens(text, seed=0, **kw, **gkw)
    for name, kw in variants:
        dt, _ = timed(lambda: eng.sample_image_tokens(text, seed=1, **kw, **gkw))
        res[f"cached_graph_{name}_tokens_per_s"] = round(R * P / dt, 1)
        res[f"cached_graph_{name}_ms_per_position"] = round(dt / P * 1e3, 4)
        res[f"cached_graph_{name}_images_per_s"] = round(R / dt, 3)
    if guided:
        return res
    k = P - plain_positions
    prefix = torch.zeros(B, k, dtype=torch.int32)
    eng.sample_image_tokens(text, seed=0, temperature=1.0, top_k=32, kv_cache=False, image_prefix=prefix[:, :P - 1])   # warm-up
    dt, _ = timed(lambda: eng.sample_image_tokens(text, seed=1, temperature=1.0, top_k=32, kv_cache=False, image_prefix=prefix))
    res["plain_top_k_tokens_per_s"] = round(B * plain_positions / dt, 1)
    res["plain_top_k_ms_per_position"] = round(dt / plain_positions * 1e3, 3)
    res["plain_positions_timed"] = plain_positions
    res["cached_over_plain"] = round(res["cached_graph_top_k_tokens_per_s"] / res["plain_top_k_tokens_per_s"], 1)
    if eng.recompute and eng._kv is not None:
        res["sampler_kv_cache_bytes"] = int(sum(t.numel() * t.element_size() for t in eng._kv))
    return res


def kv_pair_bench(eng, text, R, P, c, B, S, gkw, rounds=5):
    """the top-k sampler on the bf16 and on the fp8 cache, alternating in one process: per type the median over `rounds` timed calls"""
    import hashlib
    import statistics
    from src.dalle_mtf.kv_cache import kv_cache_bytes
    kw = dict(temperature=1.0, top_k=32, **gkw)
    times, out = {"bf16": [], "fp8": []}, {}
    for kv in times:
        for _ in range(2):                        # warm-up: caches, graph capture
            eng.sample_image_tokens(text, seed=0, kv_cache_dtype=kv, **kw)
    for _ in range(rounds):
        for kv in times:
            dt, toks = timed(lambda: eng.sample_image_tokens(text, seed=1, kv_cache_dtype=kv, **kw))
            times[kv].append(dt)
            out[kv] = dict(tokens_sha1=hashlib.sha1(toks.cpu().numpy().tobytes()).hexdigest())
    for kv, ts in times.items():
        dt = statistics.median(ts)
        out[kv].update(ms_per_position=round(dt / P * 1e3, 4), tokens_per_s=round(R * P / dt, 1),
                       ms_per_position_all=[round(t / P * 1e3, 4) for t in ts],
                       cache_bytes=kv_cache_bytes(kv, c["L"], B, S, c["d"], c["H"]))
    out["fp8_over_bf16_time"] = round(out["fp8"]["ms_per_position"] / out["bf16"]["ms_per_position"], 4)
    return out


def kernel_bench(reps):
    import dalle_hip as dh
    res = {}
    for nv in (2048, 8192):
        for B in (32, 128):
            z = (torch.randn(B, nv, device="cuda") * 2).to(torch.bfloat16)
            bias = (torch.randn(nv, device="cuda") * 0.5).to(torch.bfloat16)
            nxt = torch.empty(B, dtype=torch.int32, device="cuda")
            lp = torch.zeros(B, dtype=torch.float32, device="cuda")
            runs = (("sample_tokens top_k=32", lambda p: dh.sample_tokens(z, nv, bias, B, nv, temperature=1.0, top_k=32, seed=1, pos=p, next_tok=nxt)),
                    ("sample_tokens_p top_k=32 top_p=0.9", lambda p: dh.sample_tokens_p(z, nv, bias, B, nv, temperature=1.0, top_k=32, seed=1, top_p=0.9, pos=p, next_tok=nxt)),
                    ("sample_tokens_p top_p=0.9", lambda p: dh.sample_tokens_p(z, nv, bias, B, nv, temperature=1.0, seed=1, top_p=0.9, pos=p, next_tok=nxt)),
                    ("sample_tokens_p top_p=0.9 logp", lambda p: dh.sample_tokens_p(z, nv, bias, B, nv, temperature=1.0, seed=1, top_p=0.9, pos=p, next_tok=nxt, logp=lp)))
            for name, fn in runs:
                for p in range(reps):
                    fn(p)
                torch.cuda.synchronize()
                dt, _ = timed(lambda: [fn(p) for p in range(reps)])
                res[f"nv{nv} B{B} {name} host_us_per_launch"] = round(dt / reps * 1e6, 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES), default="example")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--plain-positions", type=int, default=16)
    ap.add_argument("--guidance-scale", dest="guidance_scale", type=float, default=1.0)
    ap.add_argument("--kv-cache-dtype", dest="kv_cache_dtype", choices=("bf16", "fp8", "both"), default=None)
    for name, (kw, _) in OPTIONS.items():
        ap.add_argument("--" + name.replace("_", "-"), dest=name, **kw)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = kernel_bench(a.reps) if a.kernels else engine_bench(a.shape, a.batch, a.plain_positions, a.guidance_scale, a.kv_cache_dtype,
                                                                     **{name: getattr(a, name) for name in OPTIONS})
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
