"""Image generation from captions: the predict path the reference leaves unfinished (src/model_fns.py:135-136 raises).

generate(argv) builds a run's DALL-E at the generation batch, restores its checkpoint and its VAE (the loading logic of
src/model_fns.py), samples image tokens on the KV-cached decode graph (DalleEngine.sample_image_tokens: temperature, top-k,
top-p, image completion, the model's log-likelihood of each sample), decodes them with the VAE and writes

    tokens.npy    int32 [N * n, image_seq_len]   row i * n + j = sample j of caption i
    captions.npy  int32 [N, text_seq_len]
    logprob.npy   float32 [N * n]                sum over the drawn tokens of log p(token) at temperature 1, unfiltered
    <i>_<j>.png   caption i, sample j (when the run has a VAE)
    generate.json the settings, the checkpoints and the timings

Rows are generated in batches of --batch (the last one padded by repeating its rows); batch j draws with seed + j, and rows
of a batch draw different noise because the counter-based noise hashes the row.  --guidance-scale S != 1 (classifier-free
guidance) pairs every row with a null-caption row in the same batch, so a batch of --batch engine rows generates --batch / 2
output rows; the files keep their shapes per caption and per sample, and logprob.npy stays the conditional model's own score.
--weights ema | raw samples from the run's weight average (config key "ema_decay") or from the raw iterate; auto (default)
takes the average when the checkpoint or the config has one.  generate.json records the resolved choice.
--kv-cache-dtype bf16 | fp8 (else the config key "kv_cache_dtype", else bf16) picks the sampler's key/value cache; with fp8
logprob.npy is the likelihood under the fp8-cache computation.  generate.json records the resolved type.
Every argument is checked before the GPU is touched."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

SOURCES = ("caption_ids", "captions", "from_eval")


def build_parser():
    from src.dalle_mtf.kv_cache import KV_CACHE_DTYPES
    p = argparse.ArgumentParser(prog="generate_dalle.py", description="Generate images from captions with a trained DALL-E run.")
    p.add_argument("--model", required=True, help="DALL-E config: a name under configs/ or a path to a .json file")
    p.add_argument("--out", default="generated", help="output directory (default: %(default)s)")
    p.add_argument("--checkpoint", default=None,
                   help="DALL-E checkpoint: a model.ckpt-<step>.pt, a run directory, or the <prefix> of a reference checkpoint "
                        "(default: the newest under the config's model_path, else its tf_checkpoint)")
    p.add_argument("--batch", type=int, default=None, help="rows per generation batch (default: the config's predict_batch_size)")
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument("--caption-ids", dest="caption_ids", default=None, help=".npy of int caption ids [N, text_seq_len]")
    src.add_argument("--captions", default=None, help="text file, one caption per line (needs the GPT-2 vocabulary locally)")
    src.add_argument("--from-eval", dest="from_eval", type=int, default=None, help="the first N captions of the eval input")
    p.add_argument("--image-prefix", dest="image_prefix", type=int, default=0,
                   help="with --from-eval: complete the eval images from their first K image tokens")
    p.add_argument("--samples-per-caption", dest="samples", type=int, default=1)
    p.add_argument("--temperature", type=float, default=1.0, help="0 = greedy")
    p.add_argument("--top-k", dest="top_k", type=int, default=0, help="0 = no top-k filter")
    p.add_argument("--top-p", dest="top_p", type=float, default=1.0, help="nucleus mass in (0, 1]; 1 = no nucleus filter")
    p.add_argument("--guidance-scale", dest="guidance_scale", type=float, default=1.0,
                   help="classifier-free guidance: draw from l_uncond + S (l_cond - l_uncond), the unconditional rows carrying the "
                        "null caption; a batch then generates --batch / 2 rows.  1 = off (default)")
    p.add_argument("--weights", choices=("auto", "ema", "raw"), default="auto",
                   help="sample from the weight average (ema), the raw iterate (raw), or the average when the run has one (auto, "
                        "default)")
    p.add_argument("--kv-cache-dtype", dest="kv_cache_dtype", choices=KV_CACHE_DTYPES, default=None,
                   help="the sampler's key/value cache: bf16, or fp8 (E4M3 with a power-of-two scale per position and head: a third "
                        "of the memory, about half the bytes read per position; logprob.npy is then the likelihood under the "
                        "fp8-cache computation).  Default: the config's kv_cache_dtype, else bf16")
    p.add_argument("--seed", type=int, default=0, help="batch j draws with seed + j")
    p.add_argument("--no-images", dest="no_images", action="store_true", help="write tokens and scores only")
    return p


def _fail(parser, msg):
    parser.error(msg)      # exits with status 2 and the usage line


def load_config(model):
    from src.utils import fetch_model_params
    params = fetch_model_params(model)
    assert (params["model_type"] or "").lower() == "dalle", f'model_type {params["model_type"]} is not dalle'
    params["vae_params"] = fetch_model_params(params["vae_model"]) if params["vae_model"] else None
    return params


def check_args(parser, args, params):
    """everything that can be refused without a GPU"""
    from src.model_fns import image_seq_len_of
    from src.dalle_mtf.kv_cache import resolve_kv_cache_dtype
    P = image_seq_len_of(params)
    if not (0.0 < args.top_p <= 1.0):
        _fail(parser, f"--top-p must lie in (0, 1] (got {args.top_p})")
    if not (args.temperature >= 0.0):
        _fail(parser, f"--temperature must be >= 0 (got {args.temperature})")
    if args.top_k < 0:
        _fail(parser, f"--top-k must be >= 0 (got {args.top_k})")
    if args.samples < 1:
        _fail(parser, f"--samples-per-caption must be >= 1 (got {args.samples})")
    if args.batch is not None and args.batch < 1:
        _fail(parser, f"--batch must be >= 1 (got {args.batch})")
    try:       # the flag goes before the config key
        args.kv_cache_dtype = resolve_kv_cache_dtype(args.kv_cache_dtype if args.kv_cache_dtype is not None else params.get("kv_cache_dtype"))
    except ValueError as e:
        _fail(parser, f"config key {e}")
    if args.batch is None and not params["predict_batch_size"]:
        _fail(parser, "--batch is needed: the config has no predict_batch_size")
    if not (args.guidance_scale >= 0.0 and math.isfinite(args.guidance_scale)):
        _fail(parser, f"--guidance-scale must be finite and >= 0 (got {args.guidance_scale})")
    if args.guidance_scale != 1.0 and (args.batch or int(params["predict_batch_size"])) % 2:
        _fail(parser, f"--guidance-scale pairs the rows of a batch, so the batch must be even "
                      f"(got {args.batch or int(params['predict_batch_size'])})")
    if not (0 <= args.image_prefix < P):
        _fail(parser, f"--image-prefix must lie in [0, image_seq_len = {P}) (got {args.image_prefix})")
    if args.image_prefix and args.from_eval is None:
        _fail(parser, "--image-prefix needs --from-eval (the prefixes are the eval images' first tokens)")
    if args.from_eval is not None and args.from_eval < 1:
        _fail(parser, f"--from-eval must be >= 1 (got {args.from_eval})")
    if args.image_prefix and params.get("synthetic_image_tokens"):
        _fail(parser, "--image-prefix needs a VAE to tokenise the eval images (the config sets synthetic_image_tokens)")
    if args.image_prefix and params.get("image_vocab_size") and params["vae_params"] and \
            params["vae_params"].get("num_tokens") and params["vae_params"]["num_tokens"] > params["image_vocab_size"]:
        _fail(parser, "--image-prefix: the VAE has more tokens than the DALL-E image vocabulary")
    for name in ("caption_ids", "captions"):
        path = getattr(args, name)
        if path is not None and not os.path.isfile(path):
            _fail(parser, f"--{name.replace('_', '-')}: {path} not found")
    if args.checkpoint is not None and not (os.path.exists(args.checkpoint) or os.path.exists(args.checkpoint + ".index")):
        _fail(parser, f"--checkpoint: {args.checkpoint} not found")
    return P


def _tokenizer(params):
    from src.data import get_tokenizer
    tok = get_tokenizer(params["tokenizer"], vocab_size=params["text_vocab_size"])
    assert len(tok) == params["text_vocab_size"], \
        f"tokenizer vocab size {len(tok)} must equal model vocab size {params['text_vocab_size']}"
    return tok


def read_captions(parser, args, params):
    """caption ids int32 [N, T] (and, for --from-eval, the eval images [N, H, W, C] in [-1, 1] or None); no GPU"""
    from src.input_fns import truncate_or_pad_label
    T = params["text_seq_len"]
    if args.caption_ids is not None:
        ids = np.load(args.caption_ids)
        if ids.ndim != 2 or ids.shape[1] != T or ids.shape[0] < 1 or not np.issubdtype(ids.dtype, np.integer):
            _fail(parser, f"--caption-ids: need an int array [N, text_seq_len = {T}] (got {ids.dtype} {ids.shape})")
        if ids.min() < 0 or ids.max() >= params["text_vocab_size"]:
            _fail(parser, f"--caption-ids: ids must lie in [0, {params['text_vocab_size']})")
        return ids.astype(np.int32), None
    if args.captions is not None:
        from src.data.tokenizer_utils import _OfflineTokenizer
        tok = _tokenizer(params)
        if isinstance(tok, _OfflineTokenizer):
            _fail(parser, "--captions: the GPT-2 vocabulary is not available locally (only the offline stand-in tokenizer "
                          "loaded), so text cannot be tokenised; pass --caption-ids with ids tokenised elsewhere")
        lines = [ln.rstrip("\n") for ln in open(args.captions, encoding="utf-8")]
        lines = [ln for ln in lines if ln.strip()]
        if not lines:
            _fail(parser, f"--captions: {args.captions} holds no caption")
        return np.stack([truncate_or_pad_label(tok.encode(ln), params) for ln in lines]).astype(np.int32), None
    from src.input_fns import dalle_input_fn
    caps, imgs = [], []
    it = dalle_input_fn(params, eval=True)
    try:
        while sum(len(c) for c in caps) < args.from_eval:
            img, cap = next(it)
            caps.append(np.asarray(cap, np.int32))
            imgs.append(np.asarray(img, np.float32))
    finally:
        if hasattr(it, "close"):
            it.close()
    return np.concatenate(caps)[:args.from_eval], np.concatenate(imgs)[:args.from_eval]


def generate(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    params = load_config(args.model)
    P = check_args(parser, args, params)
    B = args.batch or int(params["predict_batch_size"])
    params["padding_id"] = _tokenizer(params).encode("<|padding|>")[0]
    params["batch_size"] = B                      # the eval input's batch (--from-eval)
    captions, eval_images = read_captions(parser, args, params)
    N, n, K = captions.shape[0], args.samples, args.image_prefix

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("generate_dalle.py needs a GPU (MI355X)")
    import dalle_hip as dh
    from src.model_fns import _build

    t0 = time.perf_counter()
    params["predict_batch_size"] = B
    params["_tokenizer_batch"] = B                # the VAE decodes / tokenises one generation batch at a time
    params["_dalle_checkpoint"] = args.checkpoint
    st = _build(params, "predict")
    model, vae, eng = st["model"], st["vae"], st["model"].engine
    assert st["image_seq_len"] == P
    if st["restored_from"] is None:
        print("generate: no DALL-E checkpoint found (model_path / --checkpoint / tf_checkpoint): sampling from freshly "
              "initialised weights", file=sys.stderr)
    from src.dalle_mtf.ema import resolve_weights
    from src.dalle_mtf.options import report
    try:
        which = resolve_weights(args.weights, eng.ema is not None)
    except ValueError:
        raise SystemExit(f"generate_dalle.py: --weights ema: no weight average to sample from: the checkpoint "
                         f"({st['restored_from']}) carries none and the config sets no ema_decay")
    torch.cuda.synchronize()
    t_load = time.perf_counter() - t0

    prefixes = None
    if K:
        # the eval images' tokens, as training sees them (argmax of the VAE logits, src/model_fns.py:72-77)
        prefixes = np.empty((N, P), np.int32)
        T = eng.T
        buf = torch.empty(B, T + P, dtype=torch.int32, device=eng.dev)
        zero = torch.zeros(B, T, dtype=torch.int32, device=eng.dev)
        for c0 in range(0, N, B):
            m = min(B, N - c0)
            imgs = np.concatenate([eval_images[c0:c0 + m], np.repeat(eval_images[c0 + m - 1:c0 + m], B - m, 0)])
            logits = vae.forward(torch.from_numpy(imgs).to(eng.dev), return_logits=True)
            dh.assemble_tokens(zero, logits.contiguous(), buf, B, T, P, logits.shape[-1], 0)
            prefixes[c0:c0 + m] = buf[:m, T:].cpu().numpy()

    rows = N * n
    tokens = np.empty((rows, P), np.int32)
    logprob = np.empty((rows,), np.float32)
    images = []
    t_sample = t_decode = 0.0
    guided = args.guidance_scale != 1.0
    Bg = B // 2 if guided else B                  # output rows per batch: guidance spends the other half on the null caption
    nb = (rows + Bg - 1) // Bg
    for j in range(nb):
        r = np.minimum(np.arange(j * Bg, (j + 1) * Bg), rows - 1)   # the last batch repeats its last row
        cap = torch.from_numpy(captions[r // n])
        pre = torch.from_numpy(prefixes[r // n, :K]) if K else None
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        toks, lp = model.sample(cap, temperature=args.temperature, top_k=args.top_k, seed=args.seed + j, top_p=args.top_p,
                                image_prefix=pre, return_logprobs=True, guidance_scale=args.guidance_scale, weights=which,
                                kv_cache_dtype=args.kv_cache_dtype)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        m = min(Bg, rows - j * Bg)
        tokens[j * Bg:j * Bg + m] = toks[:m].cpu().numpy()
        logprob[j * Bg:j * Bg + m] = lp[:m].cpu().numpy()
        if vae is not None and not args.no_images:
            img = vae.decode_tokens(torch.cat([toks, toks]) if guided else toks)      # the VAE is built at the batch B
            images.extend(img[:m].detach().cpu())
            torch.cuda.synchronize()
        t_sample += t2 - t1
        t_decode += time.perf_counter() - t2

    os.makedirs(args.out, exist_ok=True)
    np.save(os.path.join(args.out, "tokens.npy"), tokens)
    np.save(os.path.join(args.out, "captions.npy"), captions)
    np.save(os.path.join(args.out, "logprob.npy"), logprob)
    if images:
        from src.utils.utils import pil_images
        x = torch.stack(images)
        for r, (_, pil) in enumerate(pil_images((x + 1) / 2)):     # VAE output in [-1, 1]
            pil.save(os.path.join(args.out, f"{r // n}_{r % n}.png"))
    vae_ck = (params.get("vae_checkpoint_path") or None) if vae is not None else None
    info = dict(model=args.model, checkpoint=st["restored_from"], vae_checkpoint=vae_ck, captions=int(N), samples_per_caption=n,
                rows=int(rows), batch=int(B), batches=int(nb), seed=args.seed, seeds=f"batch j draws with seed + j",
                temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, guidance_scale=args.guidance_scale, weights=which, image_prefix=K, image_seq_len=int(P),
                source=next(s for s in SOURCES if getattr(args, s) is not None), images_written=len(images),
                recompute_grad=bool(eng.recompute),
                **report(eng.options),
                seconds=dict(load=round(t_load, 3), sample=round(t_sample, 3), decode_and_copy=round(t_decode, 3)),
                tokens_per_s=round(nb * Bg * (P - K) / t_sample, 1) if t_sample > 0 else None,
                kv_cache_dtype=args.kv_cache_dtype)
    with open(os.path.join(args.out, "generate.json"), "w") as f:
        json.dump(info, f, indent=1)
    print(json.dumps(info))
    return info
