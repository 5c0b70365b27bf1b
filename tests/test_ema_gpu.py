"""Weight EMA on the MI355X: dmi_ema_step against the numpy float32 restatement bit for bit, the engine's recurrence under Adam
and Adafactor, the ema_weights() context manager (forward, decode graph, restore), checkpoints, and "ema_eval" through
dalle_model_fn."""
import numpy as np
import pytest
import torch

import ema_ref
from engine_case import P, T, build, inputs

pytestmark = pytest.mark.gpu

D, H, L = 128, 2, 2                      # the shared case (tests/engine_case.py) at this width and depth
PAD = 16                                 # sentinel elements behind n
SIZES = [1, 5, 128, 2051, 2 ** 20 + 8]
OMDS = [0.0, 1.0, 1e-3, float(np.float32(0.9))]


def _bits(t):
    a = t.detach().cpu()
    if a.dtype == torch.bfloat16:
        return a.view(torch.int16).numpy().view(np.uint16)
    return a.numpy().view(np.uint32)


def _same_bits(got, want, what):
    """bit equality; where the restatement gives NaN the kernel must give a NaN (IEEE leaves its sign and payload open)"""
    want = np.asarray(want, np.float32)
    nan = np.isnan(want)
    got_f = got.detach().cpu().float().numpy()
    assert np.array_equal(np.isnan(got_f), nan), what
    if got.dtype == torch.bfloat16:
        g, w = _bits(got), ema_ref.bf16_rne_bits(want)
    else:
        g, w = _bits(got), want.view(np.uint32)
    bad = np.flatnonzero((g != w) & ~nan)
    assert bad.size == 0, (what, bad[:8], g[bad[:8]], w[bad[:8]])


SPECIAL = [(0.0, 0.0), (0.0, 0.01), (1e-40, 0.0), (np.inf, 1.0), (-np.inf, 1.0), (np.nan, 1.0), (1.0, np.nan), (1.0, np.inf),
           (np.inf, np.inf), (3e-39, 1e-39), (-0.0, 0.0)]


def _inputs(n, seed):
    """p ~ N(0, 0.02) against ema of either sign over 1e-8 .. 1e3, with exact zeros, denormals, +-Inf and NaN sprinkled in"""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.02).astype(np.float32)
    ema = (rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-8, 3, n)).astype(np.float32)
    if n >= 128:
        ema[::7] = p[::7] + (rng.standard_normal(len(p[::7])) * 1e-4).astype(np.float32)   # an average close to its parameter
    for k, (e, q) in enumerate(SPECIAL):
        if k < n:
            i = (k * 37 + 3) % n if n >= 128 else k
            ema[i], p[i] = e, q
    return ema, p


def _one_pass():
    """elements one pass of the kernel's grid covers: 8 blocks of 256 lanes per CU, 4 elements per lane"""
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256 * 4


def _run(ema, p, omd, with_bf16=True):
    import dalle_hip as dh
    n = ema.size
    e = torch.full((n + PAD,), 7.25, dtype=torch.float32, device="cuda")
    e[:n] = torch.from_numpy(ema).cuda()
    q = torch.zeros(n + PAD, dtype=torch.float32, device="cuda")
    q[:n] = torch.from_numpy(p).cuda()
    b = torch.full((n + PAD,), -3.5, dtype=torch.bfloat16, device="cuda") if with_bf16 else None
    dh.ema_step(e, q, b, n, omd)
    torch.cuda.synchronize()
    return e, b


@pytest.mark.parametrize("n", SIZES + ["one_pass+1029"])
def test_kernel_against_the_numpy_restatement(n):
    if n == "one_pass+1029":      # more elements than one pass of the grid on this device, with a tail
        n = _one_pass() + 1029
    ema, p = _inputs(n, seed=n % 1000)
    for omd in OMDS:
        want = ema_ref.ema_step_ref(ema, p, omd)
        e, b = _run(ema, p, omd)
        _same_bits(e[:n], want, ("ema", n, omd))
        _same_bits(b[:n], want, ("ema_bf16", n, omd))
        assert bool((e[n:] == 7.25).all()) and bool((b[n:] == -3.5).all()), ("sentinels", n, omd)
        e2, none = _run(ema, p, omd, with_bf16=False)                   # without the bf16 copy: the same fp32 bits
        assert none is None and np.array_equal(_bits(e2), _bits(e)), (n, omd)
        e3, b3 = _run(ema, p, omd)                                      # twice on the same inputs: the same bits
        assert np.array_equal(_bits(e3), _bits(e)) and np.array_equal(_bits(b3), _bits(b)), (n, omd)
    # omd 0 keeps the average, omd 1 gives e - (e - p): the finite elements show that all three roundings happen
    fin = np.isfinite(ema) & np.isfinite(p)
    assert np.array_equal(ema_ref.ema_step_ref(ema, p, 0.0)[fin], ema[fin])


# ------------------------------------------------------------------------------------------------ engine
def _engine(**hp):
    return build(D, H, L, hparams=dict(lr=1e-2, warmup_steps=0, **hp))[1].engine


@pytest.fixture(scope="module")
def batches():
    return [torch.from_numpy(inputs(D, H, L, seed=s)[2]).cuda() for s in range(4)]


def _train(eng, batches, steps, start=0):
    for t in range(start, start + steps):
        eng.train_step(batches[t % len(batches)])
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def trained(batches):
    """three Adam steps at decay 0.9, and the state after them (shared, never modified by the tests that read it)"""
    eng = _engine(ema_decay=0.9)
    _train(eng, batches, 3)
    return eng, {k: (v.clone() if torch.is_tensor(v) else v) for k, v in eng.state_dict().items()}


@pytest.mark.parametrize("optimizer", ["adam", "adafactor"])
def test_engine_recurrence(batches, optimizer):
    eng, twin = _engine(ema_decay=0.99, optimizer=optimizer), _engine(optimizer=optimizer)
    assert twin.ema is None and twin.ema_b is None
    assert eng.ema.shape == eng.p.shape and eng.ema.dtype == torch.float32 and eng.ema_b.dtype == torch.bfloat16
    assert torch.equal(eng.ema, eng.p) and torch.equal(eng.ema_b, eng.pb)
    for t in range(3):
        prev, p_before = eng.ema.cpu().numpy(), eng.p.clone()
        eng.train_step(batches[t])
        twin.train_step(batches[t])
        torch.cuda.synchronize()
        assert eng.global_step == t + 1 and not torch.equal(eng.p, p_before)
        want = ema_ref.ema_step_ref(prev, eng.p.cpu().numpy(), ema_ref.one_minus_decay(0.99, t))
        _same_bits(eng.ema, want, ("ema", optimizer, t))
        _same_bits(eng.ema_b, want, ("ema_b", optimizer, t))
    assert not torch.equal(eng.ema, eng.p)
    assert np.array_equal(_bits(eng.p), _bits(twin.p)) and np.array_equal(_bits(eng.pb), _bits(twin.pb))


def test_context_manager(batches, trained):
    src, sd = trained
    eng, other, never = _engine(ema_decay=0.9), _engine(), _engine(ema_decay=0.9)
    eng.load_state_dict(sd)
    never.load_state_dict(sd)
    assert np.array_equal(_bits(eng.ema), _bits(src.ema)) and not torch.equal(eng.ema, eng.p)
    other.p.copy_(eng.ema)                               # a plain engine whose parameters are the average
    other.refresh_compute_copies(cast=True)
    tok, text = batches[0], batches[0][:, :T]
    raw = eng.sample_image_tokens(text, seed=5, kv_cache=True, weights="raw")     # the decode graph exists before entering
    assert any(k and not (k.guided or k.logp) for k in eng._dec["graphs"])       # the plain or the nucleus draw's (keys: engine.Draw)
    graphs = dict(eng._dec["graphs"])
    want_tok = other.sample_image_tokens(text, seed=5, kv_cache=True)
    other.forward(tok, need_grad=False)
    want_z, want_loss = other.z.clone(), other.loss.clone()
    eng.forward(tok, need_grad=False)
    raw_z = eng.z.clone()
    ptr = (eng.pb.data_ptr(), eng.pbt.data_ptr())
    pb0, pbt0, p0, m0, v0, ema0 = eng.pb.clone(), eng.pbt.clone(), eng.p.clone(), eng.m.clone(), eng.v.clone(), eng.ema.clone()
    with eng.ema_weights():
        eng.forward(tok, need_grad=False)
        assert torch.equal(eng.z, want_z) and torch.equal(eng.loss, want_loss) and not torch.equal(eng.z, raw_z)
        assert torch.equal(eng.sample_image_tokens(text, seed=5, kv_cache=True), want_tok)
        assert torch.equal(eng.sample_image_tokens(text, seed=5, kv_cache=True, weights="ema"), want_tok)
        assert eng._dec["graphs"] == graphs              # replayed, not captured again
        assert (eng.pb.data_ptr(), eng.pbt.data_ptr()) == ptr
        for call in (lambda: eng.train_step(tok), eng.backward, eng.optimizer_step):
            with pytest.raises(RuntimeError, match="ema_weights"):
                call()
    torch.cuda.synchronize()
    assert (eng.pb.data_ptr(), eng.pbt.data_ptr()) == ptr
    assert np.array_equal(_bits(eng.pb), _bits(pb0)) and np.array_equal(_bits(eng.pbt), _bits(pbt0))
    for a, b in ((eng.p, p0), (eng.m, m0), (eng.v, v0), (eng.ema, ema0)):
        assert np.array_equal(_bits(a), _bits(b))
    assert torch.equal(eng.sample_image_tokens(text, seed=5, kv_cache=True, weights="raw"), raw)
    assert torch.equal(eng.sample_image_tokens(text, seed=5, kv_cache=True), want_tok)      # None: the average, when there is one
    _train(eng, batches, 1, start=3)
    _train(never, batches, 1, start=3)
    assert np.array_equal(_bits(eng.p), _bits(never.p)) and np.array_equal(_bits(eng.ema), _bits(never.ema))
    with pytest.raises(ValueError, match="average"):
        with other.ema_weights():
            pass
    with pytest.raises(ValueError, match="average"):
        other.sample_image_tokens(text, seed=5, weights="ema")


def test_checkpoint_round_trip(batches, trained):
    whole = _engine(ema_decay=0.9)
    _train(whole, batches, 4)
    first = _engine(ema_decay=0.9)
    _train(first, batches, 2)
    sd = first.state_dict()
    assert sd["ema"].dtype == torch.float32 and not sd["ema"].is_cuda and "ema_b" not in sd
    second = _engine(ema_decay=0.9)
    second.load_state_dict(sd)
    assert np.array_equal(_bits(second.ema), _bits(first.ema)) and np.array_equal(_bits(second.ema_b), _bits(first.ema_b))
    _train(second, batches, 2, start=2)
    assert second.global_step == 4
    assert np.array_equal(_bits(second.p), _bits(whole.p)) and np.array_equal(_bits(second.ema), _bits(whole.ema))
    assert np.array_equal(_bits(second.ema_b), _bits(whole.ema_b))
    assert "ema" not in _engine().state_dict()
    # export under the reference's names
    ex, exp = whole.export_reference(buf=whole.ema), whole.export_reference()
    assert list(ex) == list(exp) and all(ex[k].shape == exp[k].shape for k in exp)
    name = "layer_0/attn/q"
    o = whole.lay.offset["layer_0/attn/qkv"]
    assert np.array_equal(ex[name], whole.ema[o:o + D * 3 * D].view(D, 3 * D)[:, :D].cpu().numpy()) and not np.array_equal(ex[name], exp[name])


def test_checkpoint_without_an_average_into_an_averaging_engine(batches):
    plain = _engine()
    _train(plain, batches, 2)
    sd = plain.state_dict()
    assert "ema" not in sd
    eng = _engine(ema_decay=0.9)
    eng.ema.fill_(3.0)
    eng.load_state_dict(sd)
    assert np.array_equal(_bits(eng.p), _bits(plain.p)) and np.array_equal(_bits(eng.ema), _bits(eng.p))
    assert np.array_equal(_bits(eng.ema_b), _bits(eng.pb)) and eng.global_step == 2
    prev = eng.ema.cpu().numpy()
    _train(eng, batches, 1, start=2)                     # averaging starts in mid-training, on the schedule's step 2
    _same_bits(eng.ema, ema_ref.ema_step_ref(prev, eng.p.cpu().numpy(), ema_ref.one_minus_decay(0.9, 2)), "ema after the load")


def test_checkpoint_with_an_average_into_an_engine_without_the_key(batches, trained):
    src, sd = trained
    eng, other = _engine(), _engine()
    assert eng.ema is None
    eng.load_state_dict(sd)
    assert eng.ema_decay is None and np.array_equal(_bits(eng.ema), _bits(src.ema)) and np.array_equal(_bits(eng.ema_b), _bits(src.ema_b))
    other.p.copy_(src.ema)
    other.refresh_compute_copies(cast=True)
    text = batches[1][:, :T]
    assert torch.equal(eng.sample_image_tokens(text, seed=3, weights="ema"), other.sample_image_tokens(text, seed=3))
    before, p_before = eng.ema.clone(), eng.p.clone()
    _train(eng, batches, 1, start=3)
    assert np.array_equal(_bits(eng.ema), _bits(before)) and not torch.equal(eng.p, p_before)


def test_ema_eval_through_dalle_model_fn():
    from oracle import dalle_oracle as do
    from src.model_fns import _build, dalle_model_fn
    from src.utils import ModeKeys, fetch_model_params

    def config(**kw):
        p = fetch_model_params("dalle_example")
        p.update(train_batch_size=2, eval_batch_size=2, model_path=None, n_layers=L, n_embd=D, n_heads=H, synthetic_image_tokens=P,
                 text_seq_len=T, warmup_steps=1, lr=1e-2, ema_decay=0.99, **kw)
        return p
    p = config(ema_eval=True)
    text = torch.from_numpy(do.synthetic_captions(2, T, p["text_vocab_size"], seed=3))
    img = torch.from_numpy(do.synthetic_image_tokens(2, P, 512, seed=4))
    for i in range(3):
        assert dalle_model_fn(img, text, ModeKeys.TRAIN, p).train_op() == i + 1
    eng = p["_dalle_state_train"]["model"].engine
    assert eng.ema_eval and eng.ema_decay == 0.99
    tokens = torch.cat([text, img + p["text_vocab_size"]], 1).to(device="cuda", dtype=torch.int32)
    with eng.ema_weights():
        loss_ema = float(eng.forward(tokens, need_grad=False).item())
        rows_ema = eng.loss_rows.clone()
    loss_raw = float(eng.forward(tokens, need_grad=False).item())
    assert loss_ema != loss_raw
    ev = dalle_model_fn(img, text, ModeKeys.EVAL, p)
    assert p["_dalle_state_eval"] is p["_dalle_state_train"]
    assert float(ev.loss) == loss_ema and torch.equal(eng.loss_rows, rows_ema)
    # "ema_eval": false (the default), on the same weights: the raw iterate's loss
    q = config()
    q["_dalle_state_eval"] = _build(q, "eval")
    eng_q = q["_dalle_state_eval"]["model"].engine
    assert not eng_q.ema_eval
    eng_q.load_state_dict(eng.state_dict())
    ev = dalle_model_fn(img, text, ModeKeys.EVAL, q)
    assert float(ev.loss) == loss_raw
    bad = config(ema_eval=True)
    bad["ema_decay"] = None
    with pytest.raises(ValueError, match="ema_eval"):
        _build(bad, "eval")
