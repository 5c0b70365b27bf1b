#!/usr/bin/env python
"""Records what DalleEngine and DiscreteVAE ask of libdalle_hip, so that two versions of the host code can be compared exactly.

After dh.lib() the loaded library is swapped for a proxy that notes every dmi_* call: the entry's name, the value of every
argument that is not declared c_void_p, and null / non-null ("-" / "*") for every pointer (the stream is the last one: null =
the main stream).  Calls made while a stream captures are noted like any other; graph replays make no Python calls.  Entries that take a
stream enqueue work: they form the ordered launch list.  The others (workspace sizes, plans, predicates) are host-side queries
whose order carries no meaning; they are kept as a sorted count table.

For each configuration (--list prints them) the tool builds an engine, init_params(seed=3), two train_steps on seeded tokens,
one evaluation forward and -- on the sampling configurations -- one sample_image_tokens call, and writes one JSON line: the
configuration, the launch list, the query counts and SHA-256 of p, g, loss, the evaluation logits and the sampled tokens.  To
keep the file small, calls are numbers into the sorted table of distinct calls that the file's first line holds, and a launch list is
folded: an item is a call, or [n, [items]] for n repeats in a row (`unfold` restores it).  Two runs of the same host code on
the same library give the same file; --pkg selects the tree whose `src` / `dalle_hip` packages are imported (the library
itself: DALLE_HIP_LIB).

The configurations under vae/ build a DiscreteVAE instead: init_params(seed=3), three train_steps on seeded images and Gumbel
uniforms (by default the eager warm step, the graph capture and a replay), one evaluation forward, the logits with fp32_tokens off
and on, decode_tokens of seeded ids and codebook_stats(); SHA-256 of the three losses, p, g, m, v, the evaluation loss and
reconstruction, both logits, the decoded images and index, and the statistics themselves.

    python tools/launch_trace.py --out trace.jsonl [--pkg OTHER/dalle-mtf_amd] [--only NAME ...]
"""
import argparse
import ctypes
import hashlib
import inspect
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(n_embd=128, n_layers=2, n_heads=1, text_vocab=100, image_vocab=20, T=24, P=40, B=2)
WIDE = dict(n_embd=512, n_layers=3, n_heads=4, text_vocab=500, image_vocab=120, T=64, P=192, B=2)   # the fused LayerNorm width
HEADLINE = dict(n_embd=512, n_layers=2, n_heads=4, text_vocab=50258, image_vocab=512, T=256, P=1024, B=32, global_batch_size=32,
                sample=None, evaluate=False)
SAMPLER = dict(SMALL, image_vocab=64, B=4)
SHAPES = dict(small=SMALL, wide=WIDE, headline=HEADLINE, sample=SAMPLER)    # a configuration's name starts with its shape's
VAE_TINY = dict(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch_size=2)


def configurations():
    """name -> dict(shape..., hp=..., and what to run)"""
    c = {}
    for name, hp in (("default", {}), ("recompute", dict(recompute_grad=True)), ("gelu", dict(activation_fn="gelu")),
                     ("adafactor", dict(optimizer="adafactor")), ("microbatch2", dict(num_microbatches=2)),
                     ("weight_decay", dict(weight_decay=0.01)), ("ema", dict(ema_decay=0.99)),
                     ("loss_weights", dict(text_loss_weight=1, image_loss_weight=7)),
                     ("dropout", dict(embed_dropout=0.1, residual_dropout=0.1)),
                     ("dropout_recompute", dict(embed_dropout=0.1, residual_dropout=0.1, recompute_grad=True)),
                     ("rotary_1d", dict(rotary_emb="1d"))):
        c["small/" + name] = dict(SMALL, hp=hp)
    c["small/rotary_axial"] = dict(SMALL, P=64, hp=dict(rotary_emb="axial"))
    c["small/mask"] = dict(SMALL, hp={}, masks=["causal", "local:8"])
    for name, hp in (("default", {}), ("unfused", dict(fuse_ln=False, fuse_lnbwd=False)),
                     ("lnbwd_unbatched", dict(fuse_lnbwd=True, lnbwd_batch_finish=False)), ("dropout", dict(residual_dropout=0.1)),
                     ("recompute", dict(recompute_grad=True))):
        c["wide/" + name] = dict(WIDE, hp=hp)
    c["wide/hd64"] = dict(WIDE, n_heads=8, hp={})
    c["headline/default"] = dict(HEADLINE, hp={}, env={"DALLE_DGRAD_TAIL": None})
    c["headline/dgrad_tail_0"] = dict(HEADLINE, hp={}, env={"DALLE_DGRAD_TAIL": "0"})
    for name, hp, kw in (("default", {}, {}), ("unfused_draw", {}, dict(fused_sampling=False)), ("no_graph", {}, dict(decode_graph=False)),
                         ("no_kv_cache", {}, dict(kv_cache=False)), ("nucleus_logp", {}, dict(top_p=0.9, return_logprobs=True)),
                         ("guidance", {}, dict(guidance_scale=3.0)), ("image_prefix", {}, dict(image_prefix=5)),
                         ("decode_unfused_ln", dict(decode_fuse_ln=False), {}), ("recompute", dict(recompute_grad=True), {}),
                         ("rotary_1d", dict(rotary_emb="1d"), {})):
        c["sample/" + name] = dict(SAMPLER, hp=hp, sample=kw)
    c["sample/mask"] = dict(SAMPLER, hp={}, sample={}, masks=["causal", "local:8"])
    # token shift, the gated FFN and QK normalisation, on P = 64: token shift and the axial scheme need a square image grid
    shift, glu, qk_axial = dict(token_shift=True), dict(ff_glu=True), dict(qk_norm=True, rotary_emb="axial")
    for name, hp in (("token_shift", shift), ("ff_glu_relu", glu), ("ff_glu_gelu", dict(glu, activation_fn="gelu")),
                     ("qk_norm", dict(qk_norm=True)), ("qk_norm_axial", qk_axial),
                     ("all_options", dict(shift, **glu, **qk_axial, activation_fn="gelu", embed_dropout=0.1, residual_dropout=0.1,
                                          text_loss_weight=1, image_loss_weight=7))):
        c["small/" + name] = dict(SMALL, P=64, hp=hp)
    for name, hp in (("token_shift", shift), ("ff_glu", glu), ("qk_norm_axial", qk_axial)):
        c["sample/" + name] = dict(SAMPLER, P=64, hp=hp, sample={})
    # DiscreteVAE: the shipped shapes, the layers that materialise their column matrix (unaligned channels, grids that are no power
    # of two), space_to_depth, then every option of the step on one tiny model, then the eager step
    shipped = {}
    for name in ("vae_example", "vae_coco"):
        p = json.load(open(os.path.join(ROOT, "configs", name + ".json")))
        shipped[name] = dict(num_tokens=p["num_tokens"], dimensions=p["dataset"]["image_size"], convblocks=p["convblocks"], batch_size=1)
        c["vae/" + name] = dict(model=shipped[name])
    c["vae/unaligned"] = dict(model=dict(num_tokens=64, dimensions=16, convblocks=[[2, 16], [2, 64]], batch_size=2))
    c["vae/nonpow2"] = dict(model=dict(num_tokens=64, dimensions=24, convblocks=[[2, 64], [2, 128]], batch_size=2))
    c["vae/stacked"] = dict(model=dict(num_tokens=64, dimensions=32, convblocks=[[2, 64], [2, 64]], batch_size=2, stack_factor=2))
    for name, kw in (("recompute", dict(recompute_grad=True)), ("kl", dict(kl_loss_weight=0.5, kl_anneal_steps=4)),
                     ("vq", dict(quantizer="vq")), ("vq_ema", dict(quantizer="vq", vq_ema_decay=0.99, vq_restart_after=2))):
        c["vae/tiny_" + name] = dict(model=dict(VAE_TINY, **kw))
    c["vae/vae_example_eager"] = dict(model=shipped["vae_example"], graph=False)
    c["vae/nonpow2_recompute"] = dict(model=dict(c["vae/nonpow2"]["model"], recompute_grad=True))   # residual pairs re-run in backward()
    return c


class Recorder:
    """stands in for the ctypes library object: every dmi_* entry is called through a shim that notes the call"""

    def __init__(self, lib):
        self._lib, self._shims = lib, {}
        self.reset()

        self.table = {}              # distinct call -> its number, over the whole run

    def reset(self):
        self.sequence, self.queries = [], {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("dmi_"):
            return fn
        if name not in self._shims:
            types = fn.argtypes or ()
            launch = bool(types) and types[-1] is ctypes.c_void_p

            def shim(*args):
                vals = []
                for i, a in enumerate(args):
                    if i >= len(types):
                        vals.append(repr(a))
                    elif types[i] is ctypes.c_void_p:
                        flag = "-" if a is None or (isinstance(a, int) and a == 0) else "*"      # null / non-null, runs unseparated
                        if vals and not vals[-1].strip("-*"):
                            vals[-1] += flag
                        else:
                            vals.append(flag)
                    else:
                        a = getattr(a, "value", a)
                        vals.append(a.decode() if isinstance(a, bytes) else repr(a))
                key = self.table.setdefault(name[4:] + "(" + ",".join(vals) + ")", len(self.table))
                if launch:
                    self.sequence.append(key)
                else:
                    self.queries[key] = self.queries.get(key, 0) + 1
                return fn(*args)
            self._shims[name] = shim
        return self._shims[name]


def fold(seq, longest=64):
    """seq with every run of immediate repeats of a block (up to `longest` items) as [n, [block]], greedily from the left"""
    out, i = [], 0
    while i < len(seq):
        best = (0, 1, 1)         # (items saved, period, repeats)
        for p in range(1, min(longest, (len(seq) - i) // 2) + 1):
            n = 1
            while seq[i + n * p:i + (n + 1) * p] == seq[i:i + p]:
                n += 1
            best = max(best, ((n - 1) * p, p, n))
        _, p, n = best
        out.append(seq[i] if n == 1 else [n, fold(seq[i:i + p], longest)])
        i += p * n if n > 1 else 1
    return out


def unfold(items):
    return [c for it in items for c in (unfold(it[1]) * it[0] if isinstance(it, list) else [it])]


def write(path, table, lines):
    """table: distinct call -> the number the lines use; written with the calls renumbered in sorted order"""
    calls = sorted(table)
    new = {table[c]: i for i, c in enumerate(calls)}
    with open(path, "w") as f:
        for line in [dict(shapes=SHAPES, calls=calls)] + lines:
            if "launches" in line:
                seq = [new[c] for c in line["launches"]]
                assert unfold(fold(seq)) == seq
                line = dict(line, n_launches=len(seq), launches=fold(seq), queries=sorted((new[c], n) for c, n in line["queries"].items()))
            f.write(json.dumps(line, sort_keys=True, separators=(",", ":")) + "\n")


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def run_vae(name, cfg, rec):
    import numpy as np
    import torch
    from oracle import vae_oracle as vo
    from src.vae_tf import DiscreteVAE
    rec.reset()
    vae = DiscreteVAE(mode="train", **cfg["model"])
    vae.init_params(seed=3)
    B, T, grid = vae.B, vae.num_tokens, vae.grid
    digest = {}
    for step in range(3):
        img = torch.from_numpy(vo.synthetic_images(B, vae.H, seed=20 + step)).cuda()
        noise = None if vae.vq_on else torch.from_numpy(vo.synthetic_uniforms((B, grid, grid, T), seed=30 + step))
        digest[f"loss{step}"] = sha(vae.train_step(img, 1e-3, noise=noise, graph=cfg.get("graph")))
    digest.update(p=sha(vae.p), g=sha(vae.g), m=sha(vae.m), v=sha(vae.v))
    loss, recon = vae.forward(img, return_recon_loss=True, noise=noise, need_grad=False)
    digest.update(eval_loss=sha(loss), reconstruction=sha(recon))
    for fp32 in (False, True):
        vae.fp32_tokens = fp32
        digest["logits_fp32" if fp32 else "logits"] = sha(vae.forward(img, return_logits=True))
    vae.fp32_tokens = False
    ids = torch.from_numpy(np.random.default_rng(40).integers(0, T, size=(B, grid * grid)))
    digest["decoded"] = sha(vae.decode_tokens(ids))
    stats = vae.codebook_stats()
    digest["index"] = sha(vae.index)
    torch.cuda.synchronize()
    line = dict(name=name, config=cfg, launches=list(rec.sequence), queries=dict(rec.queries), sha256=digest, codebook_stats=stats)
    del vae
    torch.cuda.empty_cache()
    return line


def run(name, cfg, rec):
    if name.startswith("vae/"):
        return run_vae(name, cfg, rec)
    import numpy as np
    import torch
    from oracle import dalle_oracle as do
    from src.dalle_mtf import masks
    from src.dalle_mtf.engine import DalleEngine
    for k, v in cfg.get("env", {}).items():     # (read when the engine is built)
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v
    T, P, B, tv, iv = cfg["T"], cfg["P"], cfg["B"], cfg["text_vocab"], cfg["image_vocab"]
    hp = dict(lr=1e-3, train_steps=1000, warmup_steps=0, gradient_clipping=1.0, **cfg["hp"])
    am = [masks.pattern_mask(m, T, P) for m in cfg["masks"]] if cfg.get("masks") else None
    rec.reset()
    eng = DalleEngine(cfg["n_embd"], cfg["n_layers"], cfg["n_heads"], tv, iv, T, P, batch_size=B,
                      global_batch_size=cfg.get("global_batch_size"), hparams=hp, attn_masks=am)
    eng.init_params(seed=3)
    rows = B * hp.get("num_microbatches", 1)
    text = do.synthetic_captions(rows, T, tv, seed=11)
    tokens = torch.from_numpy(do.assemble_tokens(text, do.synthetic_image_tokens(rows, P, iv, seed=12), tv)).cuda()
    digest = {}
    for step in range(2):
        digest[f"loss{step}"] = sha(eng.train_step(tokens))
    digest.update(p=sha(eng.p), g=sha(eng.g))
    if cfg.get("evaluate", True):
        digest["eval_loss"] = sha(eng.forward(tokens[:B], need_grad=False))
        digest["eval_logits"] = sha(eng.logits())
    kw = cfg.get("sample")
    if kw is not None:
        kw, R = dict(kw), B // 2 if "guidance_scale" in kw else B
        if "image_prefix" in kw:
            kw["image_prefix"] = torch.from_numpy(do.synthetic_image_tokens(R, P, iv, seed=13)[:, :kw["image_prefix"]].astype(np.int32))
        out = eng.sample_image_tokens(torch.from_numpy(text[:R].astype(np.int32)), temperature=1.0, top_k=8, seed=5, **kw)
        for i, t in enumerate(out if isinstance(out, tuple) else (out,)):
            digest[f"sample{i}"] = sha(t)
    torch.cuda.synchronize()
    shape = SHAPES[name.split("/")[0]]           # (the first line of the file holds the shapes: a line says what it changes)
    shown = {k: v for k, v in cfg.items() if k not in shape or shape[k] != v}
    line = dict(name=name, config=shown, launches=list(rec.sequence), queries=dict(rec.queries), sha256=digest)
    del eng
    torch.cuda.empty_cache()
    for k in cfg.get("env", {}):
        os.environ.pop(k, None)
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", help="the JSON-lines file to write")
    ap.add_argument("--pkg", default=os.path.join(ROOT, "dalle-mtf_amd"), help="the tree whose src / dalle_hip packages are traced")
    ap.add_argument("--only", nargs="*", help="configuration names, or prefixes ending in / (default: all)")
    ap.add_argument("--list", action="store_true")
    a = ap.parse_args()
    cfgs = configurations()
    if a.list or not a.out:
        print("\n".join(cfgs))
        return
    sys.path[:0] = [os.path.abspath(a.pkg), ROOT]
    import dalle_hip as dh
    real = dh.lib()
    rec = dh._lib = Recorder(real)
    # the dh.<function> names engine.py uses, each behind a counter: which of them did no configuration reach?
    named = sorted(set(re.findall(r"\bdh\.([a-z_0-9]+)\b", open(os.path.join(a.pkg, "src", "dalle_mtf", "engine.py")).read())))
    reached = set()
    for fn in [n for n in named if inspect.isfunction(getattr(dh, n, None))]:
        def counted(*args, _f=getattr(dh, fn), _n=fn, **kw):
            reached.add(_n)
            return _f(*args, **kw)
        setattr(dh, fn, counted)
    lines = []
    for name, cfg in cfgs.items():
        if not a.only or name in a.only or any(o.endswith("/") and name.startswith(o) for o in a.only):
            lines.append(run(name, cfg, rec))
            print(f"[launch_trace] {name}: {len(lines[-1]['launches'])} launches", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    write(a.out, rec.table, lines)
    if any(not line["name"].startswith("vae/") for line in lines):
        print("[launch_trace] dh wrappers named by engine.py that no configuration reached:",
              sorted(n for n in named if inspect.isfunction(getattr(dh, n, None)) and n not in reached), flush=True)


if __name__ == "__main__":
    main()
