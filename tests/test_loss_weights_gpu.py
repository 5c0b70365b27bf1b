"""Text/image loss weights on a real MI355X (DESIGN.md §4 "Loss weights"): dmi_softmax_finish_w against dmi_softmax_finish on the
same inputs (the weight reaches rowscale, rowscale_bf16 and Xs and nothing else, in the exact fix-up path too), dmi_loss_reduce
against float64, and the engine / dalle_model_fn with the config keys "text_loss_weight" / "image_loss_weight" against the fp32
oracle (tests/dalle_step_ref.py) with the weighted loss of tests/loss_weights_ref.py applied to its loss_batch."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import dalle_hip as dh  # noqa: E402  (path set up by conftest)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dalle_step_ref as sref  # noqa: E402
from engine_case import HP, inputs  # noqa: E402
from loss_weights_ref import loss_reduce_ref, weighted_loss_ref  # noqa: E402
from parity import rel_l2, save_report  # noqa: E402

DEV = "cuda"


def close(got, ref, rtol, atol, what=""):
    got, ref = got.double().cpu(), ref.double().cpu()
    err = (got - ref).abs()
    bad = err > atol + rtol * ref.abs()
    assert not bad.any(), f"{what}: {int(bad.sum())}/{bad.numel()} out of tol; max err {float(err.max()):.4g}"


# ------------------------------------------------------------------ the fused head with position weights
def _head_case(M, K, V, seed, big=None):
    """inputs of the fused softmax head, as tests/test_kernels_gpu.py builds them; `big`: rows whose label logit lies > 88 below the row
    maximum, so that the exponent overflows and the row takes the exact fix-up path"""
    g = torch.Generator().manual_seed(seed)
    Vp = (V + 127) // 128 * 128
    X = (torch.randn(M, K, generator=g)).to(torch.bfloat16)
    Wt = torch.zeros(Vp, K)
    Wt[:V] = torch.randn(V, K, generator=g) * (2.0 / math.sqrt(K))
    Wt = Wt.to(torch.bfloat16)
    bias = torch.full((Vp,), -30000.0)
    bias[:V] = torch.randn(V, generator=g) * 0.5
    bias = bias.to(torch.bfloat16)
    labels = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    if big is not None:
        for r in big:
            v_hi = (int(labels[r]) + 1) % V
            Wt[v_hi] = (X[r].float() * (200.0 / float(X[r].float().pow(2).sum()))).to(torch.bfloat16)
            Wt[int(labels[r])] = (-X[r].float() * (100.0 / float(X[r].float().pow(2).sum()))).to(torch.bfloat16)
    return X, Wt, bias, labels, Vp


def _run_head(X, Wt, bias, labels, V, Vp, dz_scale, w=None):
    """label logit -> exp-epilogue GEMM (no exponent shift: the engine's mode) -> finish; w (fp32 [period]) selects
    dmi_softmax_finish_w.  Returns host copies: E, loss_rows, rowscale, rowscale_bf16, Xs, flag."""
    M, K = X.shape
    Xd, Wd, bd, ld = X.to(DEV), Wt.to(DEV), bias.to(DEV), labels.to(DEV)
    zl = torch.empty(M, dtype=torch.float32, device=DEV)
    flag = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    dh.label_logit(Xd, K, Wd, K, bd, ld, zl, flag, M, K, V)
    nparts = dh.gemm_nt_softmax_partials(Vp)
    part = torch.full((nparts, M), float("nan"), dtype=torch.float32, device=DEV)
    E = torch.zeros(M, Vp, dtype=torch.bfloat16, device=DEV)
    dh.gemm_nt_softmax(Xd, K, Wd, K, bd, None, E, Vp, part, M, Vp, K)
    loss = torch.empty(M, dtype=torch.float32, device=DEV)
    rsc = torch.full((M,), float("nan"), dtype=torch.float32, device=DEV)
    rsb = torch.full((M,), float("nan"), dtype=torch.bfloat16, device=DEV)
    Xs = torch.full((M, K), float("nan"), dtype=torch.bfloat16, device=DEV)
    args = (part, nparts, zl, None, ld, Xd, K, Wd, K, bd, E, Vp, Vp, loss, rsc, rsb, Xs, flag, M, K, V, dz_scale)
    if w is None:
        dh.softmax_finish(*args)
    else:
        dh.softmax_finish_w(*args, w.to(DEV), w.numel())
    return E.cpu(), loss.cpu(), rsc.cpu(), rsb.cpu(), Xs.cpu(), int(flag.item())


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def _same_bits(a, b, what):
    assert torch.equal(_bits(a), _bits(b)), what


HEAD_SHAPES = [(111, 37), (256, 64)]   # ragged loads + a period that crosses the 64-row blocks; the aligned path


@pytest.mark.parametrize("M,period", HEAD_SHAPES)
def test_all_weights_one_is_bit_identical_to_the_unweighted_entry_point(M, period):
    K, V = 128, 1000
    X, Wt, bias, labels, Vp = _head_case(M, K, V, seed=M)
    base = _run_head(X, Wt, bias, labels, V, Vp, 1.0 / M)
    got = _run_head(X, Wt, bias, labels, V, Vp, 1.0 / M, w=torch.ones(period))
    assert base[5] == 0 and got[5] == 0
    for a, b, what in zip(got[:5], base[:5], ("E", "loss_rows", "rowscale", "rowscale_bf16", "Xs")):
        _same_bits(a, b, what)


def _check_weighted_against_unweighted(X, got, base, w, M, rows=None):
    """E and loss_rows carry no weight (bit-identical); rowscale_w = fl(fl(dz_scale * w) / S) against w * fl(dz_scale / S): two fp32
    roundings on one side and one on the other, each 2^-24 relative -> 2.4e-7 = 4 * 2^-24 covers them; Xs and rowscale_bf16 derive
    from the returned rowscale_w (bf16 rounding: the bounds of test_fused_softmax_head); zero weights give exact zeros."""
    E, loss, rsc, rsb, Xs, _ = got
    _same_bits(E, base[0], "E must not see the weight")
    _same_bits(loss, base[1], "loss_rows must not see the weight")
    wrow = w[torch.arange(M) % w.numel()]
    close(rsc, wrow.double() * base[2].double(), 2.4e-7, 0.0, "rowscale_w vs w * rowscale")
    close(Xs, X.float() * rsc[:, None], 1.6e-2, 1e-12, "Xs")
    close(rsb, rsc, 8e-3, 0.0, "rowscale bf16")
    zero = wrow == 0
    assert int(zero.sum()) >= 2
    assert torch.all(rsc[zero] == 0) and torch.all(rsb[zero].float() == 0) and torch.all(Xs[zero].float() == 0), \
        "zero-weight rows must be exactly 0"
    assert torch.all(rsc[~zero] > 0)


@pytest.mark.parametrize("M,period", HEAD_SHAPES)
def test_random_weights_reach_rowscale_and_xs_only(M, period):
    K, V = 128, 1000
    X, Wt, bias, labels, Vp = _head_case(M, K, V, seed=M)
    w = torch.rand(period, generator=torch.Generator().manual_seed(7 + M)) * 2.0
    w[[1, period - 1]] = 0.0
    base = _run_head(X, Wt, bias, labels, V, Vp, 1.0 / M)
    got = _run_head(X, Wt, bias, labels, V, Vp, 1.0 / M, w=w)
    assert base[5] == 0 and got[5] == 0
    _check_weighted_against_unweighted(X, got, base, w, M)


def test_rows_redone_by_the_exact_fixup_keep_their_weight():
    """rows 3, 64, 129 overflow exp(logit) (test_fused_softmax_head_overflow_rows_are_redone_exactly's construction) and are
    recomputed with the row maximum as the shift: their rowscale must be w * dz_scale / S too, and exactly 0 for w = 0."""
    M, K, V, period = 130, 128, 500, 43
    big = [3, 64, 129]
    X, Wt, bias, labels, Vp = _head_case(M, K, V, seed=11, big=big)
    w = torch.rand(period, generator=torch.Generator().manual_seed(3)) * 2.0
    w[5] = 0.0
    for r, v in zip(big, (0.5, 0.0, 1.75)):
        w[r % period] = v
    dz_scale = 0.25
    base = _run_head(X, Wt, bias, labels, V, Vp, dz_scale)
    got = _run_head(X, Wt, bias, labels, V, Vp, dz_scale, w=w)
    assert base[5] == 1 and got[5] == 1
    # the fix-up's sum is fixed-order, so the relation to the unweighted run holds for the redone rows as for all others
    _check_weighted_against_unweighted(X, got, base, w, M)
    E, loss, rsc, rsb, Xs, _ = got
    z = X.float() @ Wt.float()[:V].t() + bias.float()[:V]
    lab = labels.long()
    ref_loss = torch.logsumexp(z, -1) - z[torch.arange(M), lab]
    assert float(ref_loss[3]) > 88
    close(loss, ref_loss, 1e-4, 2e-3, "loss rows")
    wrow = w[torch.arange(M) % period]
    dz_ref = (torch.softmax(z, -1) - F.one_hot(lab, V).float()) * dz_scale * wrow[:, None]
    dz = E.float()[:, :V] * rsc[:, None]
    atol = 1e-3 * dz_scale * torch.clamp(wrow, max=1.0)[:, None]       # the existing test's noise floor, scaled down with the row
    err = (dz - dz_ref).abs()
    assert not (err > atol + 1.6e-2 * dz_ref.abs()).any(), float(err.max())
    S = torch.exp(z - z.max(-1, keepdim=True).values).sum(-1)           # the normaliser under the row-maximum shift
    close(rsc[big], (wrow * dz_scale / S)[big], 1.6e-2, 0.0, "redone rows' rowscale")
    assert float(rsc[3]) > 0 and float(rsc[129]) > 0
    assert float(rsc[64]) == 0 and float(rsb[64]) == 0 and torch.all(Xs[64].float() == 0)


@pytest.mark.parametrize("n,period,split", [(4096, 128, 15), (111, 37, 5)])
def test_loss_reduce_against_float64(n, period, split):
    """fixed-order fp32 sums of positive terms, at most n / 1024 + 14 dependent additions of 2^-24 relative error each plus the
    products' and the final scale's roundings: < 2e-6 at both sizes, inside 1e-5"""
    g = torch.Generator().manual_seed(n)
    rows = torch.rand(n, generator=g) * 9.0 + 0.05
    w = torch.rand(period, generator=g) * 2.0 + 0.01
    scale = 1.0 / 7
    out = torch.full((3,), float("nan"), dtype=torch.float32, device=DEV)
    dh.loss_reduce(rows.to(DEV), n, w.to(DEV), period, split, scale, out)
    first = out.cpu()
    ref = loss_reduce_ref(rows.numpy(), w.numpy(), split, scale)
    print("loss_reduce", n, first.tolist(), ref.tolist())
    assert np.all(np.abs(first.double().numpy() - ref) <= 1e-5 * np.abs(ref)), (first, ref)
    out.fill_(float("nan"))
    dh.loss_reduce(rows.to(DEV), n, w.to(DEV), period, split, scale, out)
    _same_bits(out.cpu(), first, "two calls must agree bit for bit")


# ------------------------------------------------------------------ engine
CFG = dict(n_embd=256, n_heads=2, n_layers=2, text_vocab=300, image_vocab=64, T=16, P=112, B=2)   # tests/parity.py::compare_step


def _engine(B=CFG["B"], **hp):
    from src.dalle_mtf.engine import DalleEngine
    c = CFG
    return DalleEngine(c["n_embd"], c["n_layers"], c["n_heads"], c["text_vocab"], c["image_vocab"], c["T"], c["P"], batch_size=B,
                       hparams=dict(HP, **hp))


def _gnorm(g):
    return math.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values()))


def _step(eng, tok):
    """forward + backward: (loss, flat gradient buffer, gradients under the reference's names, loss_parts or None)"""
    loss = float(eng.forward(tok, need_grad=True).item())
    eng.backward()
    eng.wait_grads()
    parts = None if eng.loss_parts is None else eng.loss_parts.cpu().numpy().copy()
    return loss, eng.g.clone(), eng.export_reference(eng.g), parts


@pytest.fixture(scope="module")
def case():
    """weights, tokens, the fp32 oracle's loss_batch (with autograd) and the unweighted engine's step, computed once"""
    c = CFG
    cfg, P0, tokens = inputs(c["n_embd"], c["n_heads"], c["n_layers"], c["B"], T=c["T"], P=c["P"], TV=c["text_vocab"], IV=c["image_vocab"])
    Pt = sref.leaves(P0)
    mean, loss_batch = sref.forward_loss(Pt, tokens, cfg)

    def oracle(wt, wi):
        """(loss, mean_text, mean_image, gradients) of the weighted loss; wt = None: the reference's plain mean"""
        if wt is None:
            loss, mt, mi = mean, loss_batch[:, :c["T"] - 1].mean(), loss_batch[:, c["T"] - 1:].mean()
        else:
            loss, mt, mi = weighted_loss_ref(loss_batch, c["T"], wt, wi)
        return float(loss.detach()), float(mt.detach()), float(mi.detach()), sref.gradients(loss, Pt, retain_graph=True)
    tok = torch.from_numpy(tokens).cuda()
    eng = _engine()
    eng.load_reference_params(P0)
    assert eng.pos_weight is None and eng.loss_parts is None
    plain = _step(eng, tok)
    del eng
    return dict(P0=P0, tokens=tokens, tok=tok, oracle=oracle, plain=plain)


def test_uniform_equivalent_weights_give_bit_identical_gradients(case):
    """weights (T - 1, P + 1) = (15, 113) put 1 / 128 on every position, and 1 / B is a power of two: rowscale = (1/2 * 1/128) / S
    is the unweighted 1/256 / S bit for bit, so every gradient is; the loss differs by the reduce order only"""
    eng = _engine(text_loss_weight=15, image_loss_weight=113)
    eng.load_reference_params(case["P0"])
    assert torch.all(eng.pos_weight == 1.0 / 128)
    loss, g, _, parts = _step(eng, case["tok"])
    loss0, g0, _, _ = case["plain"]
    assert torch.equal(g.view(torch.int32), g0.view(torch.int32))
    assert abs(loss - loss0) <= 1e-6 * abs(loss0), (loss, loss0)
    assert abs((15 * parts[0] + 113 * parts[1]) / 128 - loss0) <= 1e-6 * abs(loss0)


def _table(gh, go):
    return {k: rel_l2(gh[k], go[k]) for k in go}


def test_weights_1_7_against_the_weighted_oracle(case):
    """loss, every gradient tensor, gradient norm and loss_parts against the fp32 oracle with the weighted loss; bounds = the
    first-step bounds of tests/parity.py::check_report for this configuration (5e-4, 4.8e-2, 2e-3).  The unweighted comparison
    runs in the same call and both per-tensor tables are written out (profiles/loss_weights_parity.json)."""
    eng = _engine(text_loss_weight=1, image_loss_weight=7)
    eng.load_reference_params(case["P0"])
    loss, _, gh, parts = _step(eng, case["tok"])
    lo, mt, mi, go = case["oracle"](1.0, 7.0)
    loss0, _, gh0, _ = case["plain"]
    lo0, _, _, go0 = case["oracle"](None, None)
    tab, tab0 = _table(gh, go), _table(gh0, go0)
    rep = dict(config=CFG, weights=[1, 7],
               weighted=dict(loss_hip=loss, loss_oracle=lo, loss_parts_hip=parts.tolist(), loss_parts_oracle=[mt, mi],
                             grad_norm_hip=_gnorm(gh), grad_norm_oracle=_gnorm(go), grad_rel_l2=tab),
               unweighted=dict(loss_hip=loss0, loss_oracle=lo0, grad_norm_hip=_gnorm(gh0), grad_norm_oracle=_gnorm(go0),
                               grad_rel_l2=tab0))
    save_report("loss_weights_parity.json", rep)
    print({k: v for k, v in rep["weighted"].items() if k != "grad_rel_l2"}, "worst", max(tab.items(), key=lambda t: t[1]))
    print({k: v for k, v in rep["unweighted"].items() if k != "grad_rel_l2"}, "worst", max(tab0.items(), key=lambda t: t[1]))
    for r in (rep["unweighted"], rep["weighted"]):
        assert abs(r["loss_hip"] - r["loss_oracle"]) <= 5e-4 * abs(r["loss_oracle"]), r
        assert max(r["grad_rel_l2"].values()) <= 4.8e-2, sorted(r["grad_rel_l2"].items(), key=lambda t: -t[1])[:4]
        assert abs(r["grad_norm_hip"] - r["grad_norm_oracle"]) <= 2e-3 * r["grad_norm_oracle"], r
    assert abs(parts[0] - mt) <= 5e-4 * mt and abs(parts[1] - mi) <= 5e-4 * mi, (parts, mt, mi)
    assert abs(loss - (parts[0] + 7 * parts[1]) / 8) <= 1e-6 * loss


@pytest.mark.parametrize("wt,wi", [(0, 1), (1, 0)])
def test_one_modality_alone(case, wt, wi):
    eng = _engine(text_loss_weight=wt, image_loss_weight=wi)
    eng.load_reference_params(case["P0"])
    loss = float(eng.train_step(case["tok"]).item())
    parts = eng.loss_parts.cpu().numpy()
    assert eng.global_step == 1 and np.isfinite(loss) and np.isfinite(eng.grad_norm())
    assert abs(loss - parts[wi]) <= 1e-6 * abs(parts[wi]), (loss, parts)


def test_microbatched_weighted_step_equals_the_full_batch_step(case):
    """num_microbatches = 2 with weights (1, 7) against the same rows as one batch: the comparison and tolerances of
    tests/test_dalle_step_gpu.py::test_microbatched_step_equals_full_batch_step"""
    from src.dalle_mtf.engine import DalleEngine
    c = CFG
    hp = dict(lr=1e-3, train_steps=10, warmup_steps=0, text_loss_weight=1, image_loss_weight=7)
    full = DalleEngine(c["n_embd"], c["n_layers"], c["n_heads"], c["text_vocab"], c["image_vocab"], c["T"], c["P"], batch_size=2,
                       hparams=dict(hp))
    full.load_reference_params(case["P0"])
    loss_full = float(full.train_step(case["tok"]))
    g_full, parts_full = full.g.clone(), full.loss_parts.cpu().numpy().copy()
    mb = DalleEngine(c["n_embd"], c["n_layers"], c["n_heads"], c["text_vocab"], c["image_vocab"], c["T"], c["P"], batch_size=1,
                     global_batch_size=1, hparams=dict(hp, num_microbatches=2))
    mb.load_reference_params(case["P0"])
    loss_mb = float(mb.train_step(case["tok"]))
    assert mb.global_step == 1
    assert abs(loss_mb - loss_full) <= 2e-3 * abs(loss_full), (loss_mb, loss_full)
    num, den = float((mb.g - g_full).norm()), float(g_full.norm())
    assert num <= 2e-2 * den, (num, den)
    assert float((mb.p - full.p).abs().max()) <= 2.5e-3
    parts_mb = mb.loss_parts_acc.cpu().numpy()
    assert np.all(np.abs(parts_mb - parts_full) <= 2e-3 * np.abs(parts_full)), (parts_mb, parts_full)
    lo = case["oracle"](1.0, 7.0)[0]
    assert abs(loss_mb - lo) <= 1e-2 * abs(lo)


def test_evaluation_forward_returns_the_weighted_loss(case):
    eng = _engine(text_loss_weight=1, image_loss_weight=7)
    eng.load_reference_params(case["P0"])
    eng.loss3.fill_(float("nan"))
    loss = float(eng.forward(case["tok"], need_grad=False).item())
    parts = eng.loss_parts.cpu().numpy()
    lo, mt, mi, _ = case["oracle"](1.0, 7.0)
    assert abs(loss - lo) <= 5e-4 * abs(lo), (loss, lo)
    assert abs(parts[0] - mt) <= 5e-4 * mt and abs(parts[1] - mi) <= 5e-4 * mi, (parts, mt, mi)
    # loss_batch stays the unweighted per-position NLL
    lb = eng.loss_rows.view(CFG["B"], -1).cpu().numpy()
    assert abs(lb[:, 15:].mean() - mi) <= 5e-4 * mi


def test_dalle_model_fn_with_loss_weights():
    """the two config keys through dalle_model_fn (a synthetic configuration like test_dalle_model_fn_microbatching's): the loss
    falls, and the summaries carry loss_text and loss_image in train and in eval"""
    from oracle import dalle_oracle as do
    from src.model_fns import dalle_model_fn
    from src.utils import ModeKeys, fetch_model_params
    from src.utils import utils as U
    p = fetch_model_params("dalle_example")
    p.update(train_batch_size=4, eval_batch_size=4, model_path=None, n_layers=1, n_embd=256, n_heads=2, synthetic_image_tokens=112,
             text_seq_len=16, warmup_steps=1, lr=3e-3, tokens_per_mb_per_replica=256, text_loss_weight=1, image_loss_weight=7)
    text = torch.from_numpy(do.synthetic_captions(4, 16, p["text_vocab_size"], seed=3))
    imgtok = torch.from_numpy(do.synthetic_image_tokens(4, 112, 512, seed=4))
    for k in ("loss_text", "loss_image"):
        U._SUMMARIES.pop(k, None)
    losses = []
    for i in range(8):
        spec = dalle_model_fn(imgtok, text, ModeKeys.TRAIN, p)
        assert spec.train_op() == i + 1
        losses.append(float(spec.loss))
    eng = p["_dalle_state_train"]["model"].engine
    assert p["num_microbatches"] == 2 and eng.loss_weights == (1.0, 7.0)
    assert abs(losses[0] - np.log(eng.V)) < 1.0 and losses[-1] < losses[0], losses
    lt, li = float(U._SUMMARIES["loss_text"]), float(U._SUMMARIES["loss_image"])
    assert abs((lt + 7 * li) / 8 - losses[-1]) <= 1e-5 * losses[-1], (lt, li, losses[-1])
    for k in ("loss_text", "loss_image"):
        U._SUMMARIES.pop(k)
    ev = dalle_model_fn(imgtok, text, ModeKeys.EVAL, p)
    lt, li = float(U._SUMMARIES["loss_text"]), float(U._SUMMARIES["loss_image"])
    assert abs((lt + 7 * li) / 8 - float(ev.loss)) <= 1e-5 * float(ev.loss), (lt, li, float(ev.loss))
