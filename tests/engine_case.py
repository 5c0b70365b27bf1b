"""The one small engine case the per-feature tests run on: T 16 caption + P 256 image positions (a 16 x 16 grid), vocabularies
300 / 64, 3 layers, 2 heads of 128, 2 sequences, weights and tokens from the oracle's seeded generators.  A test whose shape
differs on purpose passes it as arguments.  TEST INFRASTRUCTURE, imported like parity."""
import torch

T, P, TV, IV, NL, BATCH = 16, 256, 300, 64, 3, 2
HP = dict(lr=1e-3, train_steps=1000, warmup_steps=2, gradient_clipping=1.0)
PATTERNS = ["row", "column", "conv:3"]      # one attention pattern per layer


def inputs(width=256, heads=2, layers=NL, batch=BATCH, seed=0, T=T, P=P, TV=TV, IV=IV):
    """the CPU half: (cfg, P0, tokens) -- the oracle's config, the reference-named initial weights, int32 tokens [batch, T + P]"""
    from oracle import dalle_oracle as do
    cfg = do.DalleConfig(width, TV, IV, T, P, layers, heads)
    P0 = do.init_params(cfg, seed=1234 + seed, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(batch, T, TV, seed=seed + 1), do.synthetic_image_tokens(batch, P, IV, seed=seed + 2), TV)
    return cfg, P0, tokens


def build(width=256, heads=2, layers=NL, batch=BATCH, seed=0, hparams=None, weights=None, **shape):
    """(cfg, model, P0, tokens): DALLE(...) on the GPU with P0 loaded.  hparams: keys on top of HP, a key set to "absent" is left
    out; weights: a callable (P0, cfg) -> the weights to load and return in P0's place (a feature's own tensors added); **shape:
    T / P / TV / IV overrides"""
    from src.dalle_mtf.models import DALLE
    cfg, P0, tokens = inputs(width, heads, layers, batch, seed, **shape)
    if weights is not None:
        P0 = weights(P0, cfg)
    params = {k: v for k, v in dict(HP, **(hparams or {})).items() if not (isinstance(v, str) and v == "absent")}
    model = DALLE(n_embd=width, text_vocab_size=cfg.text_vocab_size, image_vocab_size=cfg.image_vocab_size, text_seq_len=cfg.text_seq_len,
                  image_seq_len=cfg.image_seq_len, n_layers=layers, n_heads=heads, batch_size=batch, params=params)
    model.engine.load_reference_params(P0)
    return cfg, model, P0, tokens


def step(eng, tokens):
    """forward + backward without all-reduce, synchronised: (the loss tensor, a clone of the flat gradient buffer)"""
    loss = eng.forward(torch.from_numpy(tokens).cuda(), need_grad=True).clone()
    eng.backward(allreduce=False)
    torch.cuda.synchronize()
    return loss, eng.g.clone()


def step_pair(make):
    """make(False), make(True) -> (model, tokens) each, built in turn with the cache emptied between: [step(...) of the first,
    step(...) of the second], for comparisons bit for bit (recompute_grad off / on, a key false / absent)"""
    out = []
    for second in (False, True):
        model, tokens = make(second)
        out.append(step(model.engine, tokens))
        del model
        torch.cuda.empty_cache()
    return out


def decode_worst(eng, tok, fill=None, graph=True):
    """the cached decode step at every image position, fed tok's tokens after a prefill of `fill` (default: tok), against the
    image-vocabulary logits of the full forward of tok: the worst max |difference| / max |full| over the positions"""
    T, S, tv = eng.T, eng.S, eng.text_vocab_size
    eng.forward(tok, need_grad=False)
    full = eng.logits()[:, :, tv:tv + eng.image_vocab_size].clone()
    eng._prefill(tok if fill is None else fill)
    worst = 0.0
    for pos in range(T - 1, S - 1):
        z = eng.decode_step(tok[:, pos].contiguous(), pos, graph=graph).float()
        ref = full[:, pos]
        worst = max(worst, float((z - ref).abs().max() / ref.abs().max()))
    return worst


def samplers_agree(eng, text):
    """seeded top-k samples of text's captions: graph-replayed decode + draw = host-launched draw = ungraphed decode, and a guided
    sample of the first caption = its decode_graph=False twin"""
    kw = dict(temperature=1.0, top_k=8, seed=3, kv_cache=True)
    a = eng.sample_image_tokens(text, **kw)
    assert torch.equal(a, eng.sample_image_tokens(text, fused_sampling=False, **kw))
    assert torch.equal(a, eng.sample_image_tokens(text, decode_graph=False, **kw))
    kw = dict(temperature=1.0, top_k=8, seed=5, guidance_scale=3.0)
    g = eng.sample_image_tokens(text[:1], **kw)
    assert tuple(g.shape) == (1, eng.S - eng.T) and torch.equal(g, eng.sample_image_tokens(text[:1], decode_graph=False, **kw))
