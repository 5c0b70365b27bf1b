"""Padded caption positions in the loss on a real MI355X (DESIGN.md §4 "Loss: padded caption positions"): dmi_loss_mask and
dmi_loss_reduce_masked against float64 (tests/loss_mask_ref.py), dmi_softmax_finish_w at period = M, and the engine /
dalle_model_fn with the config key "loss_ignore_padding" against the fp32 oracle (tests/dalle_step_ref.py) with the masked loss
applied to its loss_batch, on tests/engine_case.py's default case."""
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dalle_hip as dh  # noqa: E402  (path set up by conftest)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dalle_step_ref as sref  # noqa: E402
from engine_case import T, TV, build, inputs, step, step_pair  # noqa: E402
from loss_mask_ref import keep_ref, masked_loss_ref, out4_ref, row_weights_ref  # noqa: E402
from loss_weights_ref import weighted_loss_ref  # noqa: E402
from parity import rel_l2  # noqa: E402

DEV = "cuda"
KEY = "loss_ignore_padding"
PAD = TV - 1          # no padding_id in the hparams: text_vocab_size - 1, what the oracle's synthetic captions are padded with


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


# ------------------------------------------------------------------ the two kernels against float64
def _labels(B, S, Tt, pad, seed, lengths=None):
    """labels [B, S] of right-padded captions of Tt tokens (label p = token p + 1; image labels lie above the text vocabulary)"""
    rng = np.random.default_rng(seed)
    lab = np.empty((B, S), np.int32)
    for b in range(B):
        n = int(rng.integers(2, Tt)) if lengths is None else lengths
        tok = np.full(Tt, pad)
        tok[:n] = rng.integers(0, pad, size=n)
        lab[b, :Tt - 1] = tok[1:]
        lab[b, Tt - 1:] = rng.integers(pad + 1, pad + 65, size=S - Tt + 1)
    return lab


@pytest.mark.parametrize("weights", [None, (1, 7)], ids=["plain", "w1_7"])
@pytest.mark.parametrize("fill", ["random", "all_padded", "none_padded"])
@pytest.mark.parametrize("B,S,Tt", [(3, 24, 8), (5, 272, 16)])      # M = 72: a ragged last 64-row block; M = 1360: threads loop
def test_kernels_against_float64(B, S, Tt, fill, weights):
    """counts exact; ignored rows exactly 0; kept rows within 2.4e-7 = 4 * 2^-24 relative (the float conversions of ct and of the
    count, and the division); out4 within the 1e-5 relative of test_loss_reduce_against_float64 (the same tree); equal bits twice"""
    M, split, pad = B * S, Tt - 1, 41
    lab = _labels(B, S, Tt, pad, seed=M, lengths={"random": None, "all_padded": 1, "none_padded": Tt}[fill])
    keep, n_t, n_i = keep_ref(lab, split, pad)
    if fill == "random":      # precondition: at least one kept and one ignored text label
        assert 0 < n_t < B * split
    else:
        assert n_t == (0 if fill == "all_padded" else B * split)
    ref = row_weights_ref(lab, split, pad, weights)
    ct, ci = (1.0, 1.0) if weights is None else (weights[0] / sum(weights), weights[1] / sum(weights))
    labd = torch.from_numpy(lab).to(DEV)
    rows = torch.rand(M, generator=torch.Generator().manual_seed(M)) * 9.0 + 0.05
    rowsd = rows.to(DEV)
    scale = 1.0 / 3

    def run():
        counts = torch.full((2,), -7, dtype=torch.int32, device=DEV)
        row_w = torch.full((M,), float("nan"), dtype=torch.float32, device=DEV)
        out4 = torch.full((4,), float("nan"), dtype=torch.float32, device=DEV)
        dh.loss_mask(labd, M, S, split, pad, ct, ci, weights is None, counts, row_w)
        dh.loss_reduce_masked(rowsd, row_w, labd, M, S, split, pad, counts, scale, out4)
        return counts.cpu(), row_w.cpu(), out4.cpu()
    counts, row_w, out4 = run()
    assert counts.tolist() == [n_t, n_i], (counts, n_t, n_i)
    w = row_w.double().numpy().reshape(B, S)
    assert np.all(w[~keep] == 0.0), "ignored rows must be exactly 0"
    err = np.abs(w - ref)
    print("loss_mask", (B, S, Tt), fill, weights, "max rel err", float((err[keep] / ref[keep]).max()))
    assert np.all(err[keep] <= 2.4e-7 * ref[keep]), float((err[keep] / ref[keep]).max())
    o4 = out4_ref(rows.double().numpy().reshape(B, S), lab, split, pad, weights, scale)
    print("loss_reduce_masked", out4.tolist(), o4.tolist())
    assert np.all(np.abs(out4.double().numpy() - o4) <= 1e-5 * np.abs(o4)), (out4, o4)
    again = run()
    for a, b, what in zip(again, (counts, row_w, out4), ("counts", "row_w", "out4")):
        assert torch.equal(_bits(a), _bits(b)), f"{what}: two calls must agree bit for bit"


# ------------------------------------------------------------------ softmax_finish_w at period = M
def test_softmax_finish_w_with_period_m_equals_the_tiled_period_s():
    """what the gradient path leans on: weights that repeat every S given as [S] with period S, or tiled to [M] with period M,
    produce the same bits in rowscale, rowscale_bf16, Xs and E (M = 72: the last 64-row block is ragged)"""
    B, S, K, V = 3, 24, 128, 1000
    M, Vp = B * S, 1024
    g = torch.Generator().manual_seed(72)
    X = torch.randn(M, K, generator=g).to(torch.bfloat16).to(DEV)
    Wt = torch.zeros(Vp, K)
    Wt[:V] = torch.randn(V, K, generator=g) * (2.0 / math.sqrt(K))
    Wt = Wt.to(torch.bfloat16).to(DEV)
    bias = torch.full((Vp,), -30000.0)
    bias[:V] = torch.randn(V, generator=g) * 0.5
    bias = bias.to(torch.bfloat16).to(DEV)
    labels = torch.randint(0, V, (M,), generator=g, dtype=torch.int32).to(DEV)
    w = torch.rand(S, generator=g) * 2.0
    w[[1, 5, S - 1]] = 0.0

    def run(weight):
        zl = torch.empty(M, dtype=torch.float32, device=DEV)
        flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
        dh.label_logit(X, K, Wt, K, bias, labels, zl, flag, M, K, V)
        nparts = dh.gemm_nt_softmax_partials(Vp)
        part = torch.full((nparts, M), float("nan"), dtype=torch.float32, device=DEV)
        E = torch.zeros(M, Vp, dtype=torch.bfloat16, device=DEV)
        dh.gemm_nt_softmax(X, K, Wt, K, bias, None, E, Vp, part, M, Vp, K)
        loss = torch.empty(M, dtype=torch.float32, device=DEV)
        rsc = torch.full((M,), float("nan"), dtype=torch.float32, device=DEV)
        rsb = torch.full((M,), float("nan"), dtype=torch.bfloat16, device=DEV)
        Xs = torch.full((M, K), float("nan"), dtype=torch.bfloat16, device=DEV)
        dh.softmax_finish_w(part, nparts, zl, None, labels, X, K, Wt, K, bias, E, Vp, Vp, loss, rsc, rsb, Xs, flag, M, K, V, 0.25,
                            weight.to(DEV), weight.numel())
        assert int(flag.item()) == 0
        return rsc.cpu(), rsb.cpu(), Xs.cpu(), E.cpu()
    a, b = run(w), run(w.repeat(B))
    for x, y, what in zip(a, b, ("rowscale", "rowscale_bf16", "Xs", "E")):
        assert torch.equal(_bits(x), _bits(y)), what
    zero = (w.repeat(B) == 0)
    assert torch.all(b[0][zero] == 0) and torch.all(b[2][zero].float() == 0) and torch.all(b[0][~zero] > 0)


# ------------------------------------------------------------------ the engine against the fp32 oracle
W17 = dict(text_loss_weight=1, image_loss_weight=7)


def _gnorm(g):
    return math.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))


def _labels_of(tokens, cfg):
    from oracle import dalle_oracle as do
    return do.shift_labels(np.asarray(tokens), cfg.eos_token_id)


@pytest.fixture(scope="module")
def case():
    """the default case's fp32 oracle forward (loss_batch with autograd), computed once and never modified, and the key-off
    engine's evaluation loss_rows"""
    cfg, P0, tokens = inputs()
    labels = _labels_of(tokens, cfg)
    keep, n_t, _ = keep_ref(labels, T - 1, PAD)
    assert [int(k) for k in keep[:, :T - 1].sum(1)] == [7, 4] and n_t == 11     # captions of 8 and 5 tokens: 11 of 30 labels kept
    Pt = sref.leaves(P0)
    mean, loss_batch = sref.forward_loss(Pt, tokens, cfg)

    def oracle(weights):
        """(loss, L_t, L_i, gradients) of the masked loss"""
        loss, lt, li, frac = masked_loss_ref(loss_batch, labels, T, PAD, weights)
        assert frac == 11 / 30
        return float(loss.detach()), float(lt.detach()), float(li.detach()), sref.gradients(loss, Pt, retain_graph=True)

    def unmasked(weights):
        return float((mean if weights is None else weighted_loss_ref(loss_batch, T, *weights)[0]).detach())
    _, off, _, _ = build()
    assert off.engine.row_w is None and off.engine.text_kept_frac is None
    off.engine.forward(torch.from_numpy(tokens).cuda(), need_grad=False)
    rows_off = off.engine.loss_rows.clone()
    del off
    return dict(cfg=cfg, P0=P0, tokens=tokens, labels=labels, keep=keep, plain=float(mean.detach()), unmasked=unmasked, oracle=oracle,
                rows_off=rows_off)


@pytest.mark.parametrize("weights", [None, (1, 7)], ids=["key_alone", "key_and_w1_7"])
def test_engine_step_against_the_masked_oracle(case, weights):
    """loss, every gradient tensor, gradient norm, loss_parts and text_kept_frac against the fp32 oracle with the masked loss;
    bounds = the first-step bounds of tests/parity.py::check_report for this configuration (5e-4, 4.8e-2, 2e-3), as
    test_weights_1_7_against_the_weighted_oracle uses them.  Without the feature the engine returns the plain (or weighted) loss
    over all positions, which lies far outside the bound (asserted on the oracle's plain loss)."""
    lo, lt, li, go = case["oracle"](weights)
    # precondition: the mask matters here -- the unmasked losses (the plain mean, and the weighted one a tree without the feature
    # would return for these keys) lie at least five bounds away from the masked one
    for unmasked in (case["plain"], case["unmasked"](weights)):
        assert abs(unmasked - lo) > 5 * 5e-4 * abs(lo), (unmasked, lo)
    _, model, _, tokens = build(hparams=dict({KEY: True}, **(W17 if weights else {})))
    eng = model.engine
    assert eng.loss_ignore_padding and eng.loss_pad_id == PAD and eng.pos_weight is None
    loss = float(step(eng, tokens)[0].item())
    gh = eng.export_reference(eng.g)
    parts, frac = eng.loss_parts.cpu().numpy(), float(eng.text_kept_frac.item())
    assert eng.mask_counts.tolist() == [11, 2 * 257]
    tab = {k: rel_l2(gh[k], go[k]) for k in go}
    worst = max((e, k) for k, e in tab.items())
    gn_h, gn_o = _gnorm(gh), _gnorm(go)
    print(f"loss_ignore_padding weights {weights}: loss {loss} oracle {lo} (plain {case['plain']}); parts {parts.tolist()} oracle "
          f"{[lt, li]}; worst gradient {worst}; grad norm {gn_h} oracle {gn_o}; kept {frac}", flush=True)
    assert abs(loss - lo) <= 5e-4 * abs(lo), (loss, lo)
    assert worst[0] <= 4.8e-2, sorted(tab.items(), key=lambda t: -t[1])[:4]
    assert abs(gn_h - gn_o) <= 2e-3 * gn_o, (gn_h, gn_o)
    assert abs(parts[0] - lt) <= 5e-4 * lt and abs(parts[1] - li) <= 5e-4 * li, (parts, lt, li)
    assert abs(frac - 11 / 30) <= 1e-6
    # loss_rows stays the unmasked NLL of every position
    lb = eng.loss_rows.view(2, -1).cpu().numpy()
    assert abs(lb.mean() - case["plain"]) <= 5e-4 * case["plain"]
    # the ignored rows reach neither gradient product: their rowscale and their rows of Xs are exactly zero, so no row sends the
    # padding id, as a label, into the head's weight, bias or input gradient
    ign = torch.from_numpy(~case["keep"].reshape(-1))
    assert int(ign.sum()) == 19
    xs, rsc = eng.xs.float().cpu(), eng.rowscale.cpu()
    assert torch.all(xs[ign] == 0) and torch.all(rsc[ign] == 0) and torch.all(eng.rowscale_bf[:eng.M].float().cpu()[ign] == 0)
    assert torch.all(rsc[~ign] > 0) and torch.all(xs[~ign].abs().sum(1) > 0)


def test_an_all_null_batch_keeps_the_image_term():
    """every caption all padding (n_t = 0) with weights (1, 7): L_t = 0, nothing is renormalised, loss = 7/8 L_i, finite gradients"""
    _, model, _, tokens = build(hparams=dict({KEY: True}, **W17))
    eng = model.engine
    tokens = tokens.copy()
    tokens[:, :T] = PAD
    loss = float(step(eng, tokens)[0].item())
    parts = eng.loss_parts.cpu().numpy()
    assert eng.mask_counts.tolist() == [0, 2 * 257] and float(eng.text_kept_frac.item()) == 0.0
    assert parts[0] == 0.0 and math.isfinite(loss) and parts[1] > 0
    assert abs(loss - 7 / 8 * parts[1]) <= 1e-6 * loss, (loss, parts)
    assert bool(torch.isfinite(eng.g).all()) and float(eng.g.abs().max()) > 0
    assert torch.all(eng.rowscale.view(2, -1)[:, :T - 1] == 0)


def test_microbatched_step_is_the_mean_of_the_masked_steps(case):
    """B = 4 as two micro-batches of 2 (they keep 11 and 14 labels): every micro-batch is normalised by its own counts, so the
    step equals the mean of the two single-forward steps' masked losses and gradients; the comparison and tolerances of
    test_microbatched_weighted_step_equals_the_full_batch_step"""
    hp = dict({KEY: True}, lr=1e-3, train_steps=10, warmup_steps=0, **W17)
    cfg, one, P0, tok4 = build(batch=2, hparams=hp)
    _, _, tok4 = inputs(batch=4)
    keep4 = keep_ref(_labels_of(tok4, cfg), T - 1, PAD)[0][:, :T - 1]
    assert [int(keep4[:2].sum()), int(keep4[2:].sum())] == [11, 14]
    eng = one.engine
    halves = []
    for i in range(2):
        loss, g = step(eng, tok4[2 * i:2 * i + 2])
        halves.append((float(loss.item()), g, eng.loss_parts.cpu().numpy().copy(), float(eng.text_kept_frac.item())))
    loss_ref = (halves[0][0] + halves[1][0]) / 2
    g_ref = (halves[0][1] + halves[1][1]) / 2
    parts_ref = (halves[0][2] + halves[1][2]) / 2
    eng.g.copy_(g_ref)                     # the optimizer step on the mean gradient, as train_step ends
    eng.reducer.ready(0, eng.lay.total)
    eng.optimizer_step()
    _, mbm, _, _ = build(batch=2, hparams=dict(hp, num_microbatches=2))
    mb = mbm.engine
    loss_mb = float(mb.train_step(torch.from_numpy(tok4).cuda()))
    assert mb.global_step == 1
    assert abs(loss_mb - loss_ref) <= 2e-3 * abs(loss_ref), (loss_mb, loss_ref)
    num, den = float((mb.g - g_ref).norm()), float(g_ref.norm())
    assert num <= 2e-2 * den, (num, den)
    assert float((mb.p - eng.p).abs().max()) <= 2.5e-3
    parts_mb = mb.loss_parts_acc.cpu().numpy()
    assert np.all(np.abs(parts_mb - parts_ref) <= 2e-3 * np.abs(parts_ref)), (parts_mb, parts_ref)
    assert abs(float(mb.text_kept_frac_acc.item()) - 25 / 60) <= 1e-6
    assert abs(halves[0][3] - 11 / 30) <= 1e-6 and abs(halves[1][3] - 14 / 30) <= 1e-6


@pytest.mark.parametrize("weights", [None, (1, 7)], ids=["key_alone", "key_and_w1_7"])
def test_evaluation_forward_returns_the_masked_loss(case, weights):
    _, model, _, tokens = build(hparams=dict({KEY: True}, **(W17 if weights else {})))
    eng = model.engine
    eng.loss4.fill_(float("nan"))
    loss = float(eng.forward(torch.from_numpy(tokens).cuda(), need_grad=False).item())
    parts = eng.loss_parts.cpu().numpy()
    lo, lt, li, _ = case["oracle"](weights)
    assert abs(loss - lo) <= 5e-4 * abs(lo), (loss, lo)
    assert abs(parts[0] - lt) <= 5e-4 * lt and abs(parts[1] - li) <= 5e-4 * li, (parts, lt, li)
    assert abs(float(eng.text_kept_frac.item()) - 11 / 30) <= 1e-6
    # loss_batch stays unmasked: the key-off run's, bit for bit
    assert torch.equal(_bits(eng.loss_rows), _bits(case["rows_off"]))


@pytest.mark.parametrize("weights", [None, (1, 7)], ids=["no_weights", "w1_7"])
def test_key_false_is_the_key_absent(weights):
    """"loss_ignore_padding": false against the key absent, with and without loss weights: loss and flat gradient bit for bit"""
    w = W17 if weights else {}

    def make(absent):
        _, model, _, tokens = build(hparams=dict({KEY: "absent" if absent else False}, **w))
        assert model.engine.row_w is None and not model.engine.loss_ignore_padding
        return model, tokens
    (la, ga), (lb, gb) = step_pair(make)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(ga), _bits(gb))


def test_dalle_model_fn_with_the_key_on():
    """the key through dalle_model_fn on the small configuration of test_dalle_model_fn_with_loss_weights (two micro-batches of 2,
    weights (1, 7)): the loss falls, and loss_text, loss_image and text_kept_frac are reported in train and in eval, consistent
    with the loss (linear in the parts, so the mean over micro-batches keeps the relation)"""
    from oracle import dalle_oracle as do
    from src.model_fns import dalle_model_fn
    from src.utils import ModeKeys, fetch_model_params
    from src.utils import utils as U
    p = fetch_model_params("dalle_example")
    p.update(train_batch_size=4, eval_batch_size=4, model_path=None, n_layers=1, n_embd=256, n_heads=2, synthetic_image_tokens=112,
             text_seq_len=16, warmup_steps=1, lr=3e-3, tokens_per_mb_per_replica=256, text_loss_weight=1, image_loss_weight=7,
             loss_ignore_padding=True)
    cap = do.synthetic_captions(4, 16, p["text_vocab_size"], seed=3)
    pad = p["text_vocab_size"] - 1
    kept = (cap[:, 1:] != pad).sum(1)
    frac = float(np.mean([kept[:2].sum() / 30, kept[2:].sum() / 30]))
    assert 0 < kept.sum() < 60
    text = torch.from_numpy(cap)
    imgtok = torch.from_numpy(do.synthetic_image_tokens(4, 112, 512, seed=4))
    keys = ("loss_text", "loss_image", "text_kept_frac")
    for k in keys:
        U._SUMMARIES.pop(k, None)
    losses = []
    for i in range(8):
        spec = dalle_model_fn(imgtok, text, ModeKeys.TRAIN, p)
        assert spec.train_op() == i + 1
        losses.append(float(spec.loss))
    eng = p["_dalle_state_train"]["model"].engine
    assert p["num_microbatches"] == 2 and eng.loss_ignore_padding and eng.loss_pad_id == pad and eng.loss_weights == (1.0, 7.0)
    assert losses[-1] < losses[0], losses
    lt, li, fr = (float(U._SUMMARIES[k]) for k in keys)
    assert abs((lt + 7 * li) / 8 - losses[-1]) <= 1e-5 * losses[-1], (lt, li, losses[-1])
    assert abs(fr - frac) <= 1e-6, (fr, frac)
    for k in keys:
        U._SUMMARIES.pop(k)
    ev = dalle_model_fn(imgtok, text, ModeKeys.EVAL, p)
    lt, li, fr = (float(U._SUMMARIES[k]) for k in keys)
    assert abs((lt + 7 * li) / 8 - float(ev.loss)) <= 1e-5 * float(ev.loss), (lt, li, float(ev.loss))
    assert abs(fr - frac) <= 1e-6 and abs(float(ev.eval_metrics["text_kept_frac"]) - frac) <= 1e-6
