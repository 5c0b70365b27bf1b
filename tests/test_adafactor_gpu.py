"""Adafactor on the MI355X (src/optimizers.py:91-97; csrc/optim.hip, dmi_adafactor_step): the kernels against the float64
restatement tests/adafactor_ref.py ([MTF-RECALL]: restated from memory of mesh-tensorflow 0.1.18), the engine against the
reference-over-shim fixture tests/golden/ref_callsite_adafactor.npz and against the float64 path, determinism, checkpoints and
the command line.  Reads only committed fixtures."""
import json
import math
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, HERE)
import adafactor_ref as ar  # noqa: E402
import dalle_hip as dh  # noqa: E402
from oracle import dalle_oracle as do  # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "ref_callsite_adafactor.npz")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


# ---------------------------------------------------------------------------------------------------- kernel vs float64
# (name, shape, leading dimension, column offset inside its row block): the q/k/v-like blocks share one [256, 768] region
KVARS = [("fact_d0_rows", (300, 130), 131, None),          # d0 = axis 0, ld not a multiple of 4
         ("fact_d0_cols_pad", (130, 517), 520, None),      # d0 = axis 1, 3 pad columns
         ("blk_q", (256, 256), 768, 0), ("blk_k", (256, 256), 768, 256), ("blk_v", (256, 256), 768, 512),   # square, column blocks
         ("unfact_2d", (5, 300), 300, None),               # d1 = 5 < 128
         ("vec77", (77,), 77, None),
         ("bias_pad", (1000,), 1024, None),                # 24 pad entries
         ("wte_like", (200, 128), 128, None)]              # rows of zero gradient
SENTINEL = -30000.0


def _kernel_layout():
    off, layout, blk = 0, [], None
    for name, shp, ld, c0 in KVARS:
        R = shp[0] if len(shp) == 2 else 1
        if c0 is not None:
            if c0 == 0:
                blk = off
                off += R * ld
            layout.append((name, shp, blk + c0, ld))
        else:
            layout.append((name, shp, off, ld))
            off += ((R * ld + 127) // 128) * 128
    return layout, off


def _run_kernel(steps, clip, decay, beta1, seed=0, gscale=1.0):
    rng = np.random.default_rng(seed)
    layout, n = _kernel_layout()
    p = np.full(n, SENTINEL, np.float32)
    g = np.full(n, 7.0, np.float32)                  # garbage outside the variables: must be neither read into sums nor written
    rows, so, slot_at = [], 0, {}
    W0 = OrderedDict()
    for name, shp, off, ld in layout:
        R, C = (1, shp[0]) if len(shp) == 1 else shp
        w = rng.standard_normal((R, C)).astype(np.float32) * 0.05
        for r in range(R):
            p[off + r * ld: off + r * ld + C] = w[r]
        W0[name] = w.reshape(shp)
        fd = ar.factored_dims(shp)
        if fd is not None:
            slot_at[name] = (so, so + ((R + 3) // 4) * 4)
            rows.append([off, R, C, ld, 1, int(fd[0] == 1), so, so + ((R + 3) // 4) * 4, 0])
            so += ((R + 3) // 4) * 4 + ((C + 3) // 4) * 4
        else:
            slot_at[name] = (so,)
            rows.append([off, R, C, ld, 0, 0, 0, 0, so])
            so += ((R * C + 3) // 4) * 4
    table = torch.zeros(len(rows), dh.AF_FIELDS, dtype=torch.int64)
    table[:, :9] = torch.tensor(rows)
    totals = dh.adafactor_plan(table)
    dev = torch.device("cuda")
    P = torch.from_numpy(p).to(dev)
    M = torch.zeros(n, dtype=torch.float32, device=dev) if beta1 else None
    PB = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    S = torch.zeros(max(so, 4), dtype=torch.float32, device=dev)
    gn = torch.zeros(1, dtype=torch.float32, device=dev)
    ws = torch.empty(totals[2], dtype=torch.uint8, device=dev)
    tdev = table.to(dev)
    Wref = OrderedDict((k, v.astype(np.float64)) for k, v in W0.items())
    slots = ar.init_slots(OrderedDict((k, v.shape) for k, v in W0.items()), beta1)
    lr = 0.05
    for step in range(steps):
        gg = g.copy()
        G = OrderedDict()
        for name, shp, off, ld in layout:
            R, C = (1, shp[0]) if len(shp) == 1 else shp
            x = (rng.standard_normal((R, C)) * rng.uniform(0.1, 2.0, size=(R, 1)) * gscale).astype(np.float32)
            if name == "wte_like":
                x[::3] = 0.0                                # unused tokens
            for r in range(R):
                gg[off + r * ld: off + r * ld + C] = x[r]
            G[name] = x.reshape(shp)
        dh.adafactor_step(tdev, len(rows), totals, P, torch.from_numpy(gg).to(dev), M, S, PB, gn, clip, lr, decay, beta1, 1e-30,
                          1e-3, ws)
        norm = math.sqrt(sum(float(np.sum(v.astype(np.float64) ** 2)) for v in G.values()))
        mult = clip / max(norm, clip) if clip > 0 else 1.0
        Wref = ar.apply_grads(Wref, OrderedDict((k, v.astype(np.float64) * mult) for k, v in G.items()), slots, lr, decay, beta1)
    torch.cuda.synchronize()
    return dict(layout=layout, p=P.cpu().numpy(), p0=p, pb=PB.float().cpu().numpy(), S=S.cpu().numpy(),
                m=None if M is None else M.cpu().numpy(), gn=float(gn.item()), norm=norm, mult=mult, W0=W0, Wref=Wref, slots=slots,
                slot_at=slot_at)


def _unpack(res, name, shp, off, ld, buf):
    R, C = (1, shp[0]) if len(shp) == 1 else shp
    return np.stack([buf[off + r * ld: off + r * ld + C] for r in range(R)]).reshape(shp)


@pytest.mark.parametrize("clip,decay,beta1,gscale", [(1.0, 0.0, 0.9, 1.0),      # clip active (norm >> 1)
                                                     (1e4, 0.3, 0.9, 1.0),      # clip inactive, second-moment history
                                                     (0.0, 0.0, 0.0, 1e-3),     # no clip, no momentum slot
                                                     (0.5, 0.5, 0.5, 1e-4)])    # clip inactive: norm below it
def test_kernel_matches_float64(clip, decay, beta1, gscale):
    res = _run_kernel(steps=3, clip=clip, decay=decay, beta1=beta1, gscale=gscale)
    assert res["gn"] == pytest.approx(res["norm"] ** 2, rel=1e-5)
    if clip == 1.0:
        assert res["mult"] < 0.1
    if clip == 0.5:
        assert res["mult"] == 1.0
    covered = np.zeros(res["p"].shape, bool)
    for name, shp, off, ld in res["layout"]:
        w = _unpack(res, name, shp, off, ld, res["p"])
        R, C = (1, shp[0]) if len(shp) == 1 else shp
        for r in range(R):
            covered[off + r * ld: off + r * ld + C] = True
        up, up_ref = w - res["W0"][name], res["Wref"][name] - res["W0"][name]
        assert _rel(up, up_ref) < 1e-5, (name, _rel(up, up_ref))
        pb = _unpack(res, name, shp, off, ld, res["pb"])
        assert np.array_equal(pb, torch.from_numpy(w).bfloat16().float().numpy()), name
        sa = res["slot_at"][name]
        if len(sa) == 2:
            fd = ar.factored_dims(shp)
            vrow, vcol = res["S"][sa[0]:sa[0] + R], res["S"][sa[1]:sa[1] + C]
            vr, vc = (vrow, vcol) if fd[0] == 1 else (vcol, vrow)
            assert _rel(vr, res["slots"][name + "_slot_vr"]) < 1e-5, name
            assert _rel(vc, res["slots"][name + "_slot_vc"]) < 1e-5, name
        else:
            v = res["S"][sa[0]:sa[0] + R * C].reshape(shp)
            assert _rel(v, res["slots"][name + "_slot_v"]) < 1e-5, name
        if beta1:
            m = _unpack(res, name, shp, off, ld, res["m"])
            assert _rel(m, res["slots"][name + "_slot_m"]) < 1e-5, name
    # pad columns, pad bias entries, gaps: bit-unchanged (p), never written (m, bf16 copy)
    assert np.array_equal(res["p"][~covered].view(np.uint32), res["p0"][~covered].view(np.uint32))
    assert not np.any(res["pb"][~covered])
    if beta1:
        assert not np.any(res["m"][~covered])
    # rows of zero gradient: no update where momentum is empty
    if not beta1:
        name, shp, off, ld = [x for x in res["layout"] if x[0] == "wte_like"][0]
        w = _unpack(res, name, shp, off, ld, res["p"])
        assert np.array_equal(w[::3], res["W0"][name][::3])


def test_kernel_is_deterministic():
    a = _run_kernel(steps=2, clip=1.0, decay=0.2, beta1=0.9, seed=3)
    b = _run_kernel(steps=2, clip=1.0, decay=0.2, beta1=0.9, seed=3)
    for k in ("p", "pb", "S", "m"):
        assert np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k]), k


# ---------------------------------------------------------------------------------------------------- engine
def _engine(cfg, B, hp, P0):
    from src.dalle_mtf.engine import DalleEngine
    eng = DalleEngine(cfg.n_embd, cfg.n_layers, cfg.n_heads, cfg.text_vocab_size, cfg.image_vocab_size, cfg.text_seq_len,
                      cfg.image_seq_len, batch_size=B, hparams=dict(hp))
    eng.load_reference_params(P0)
    return eng


def _gen():
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_adafactor_golden", os.path.join(HERE, "golden", "make_adafactor_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen


@pytest.mark.parametrize("name", ["a", "b"])
def test_engine_matches_the_reference_over_shim(name):
    """three engine steps (bf16 compute) against the fixture: every variable's update and every slot by reference name.
    Factored variables (and their vr / vc / m): 0.12 relative L2 -- the later-step gradient tolerance of tests/test_dalle_step_gpu.py
    (0.092) with room for three steps of it; a slot of squares counts at half its error.  Unfactored variables (the 1-D ones, wpe
    [16, 128]): 0.35 -- with decay 0 (0.01) their x = gc / sqrt(gc^2 + eps1) is +-1 per element, so an element whose gradient is
    below the bf16 gradient noise flips sign and moves by twice the step: measured 0.19-0.23 on LayerNorm gains / biases.  The
    optimizer itself is checked exactly on the engine's own gradients by test_engine_against_the_float64_path."""
    gen = _gen()
    z = np.load(FIXTURE)
    case = gen.CASES[name]
    cfg, weights, tokens = gen.case_inputs(case)
    eng = _engine(cfg, case["batch"], case["hp"], weights)
    assert eng.optimizer == "adafactor" and (eng.m is None) == (case["hp"]["beta_1"] == 0.0) and eng.v is None
    eng.global_step = case["step"]
    tok = torch.from_numpy(tokens).cuda()
    losses = [float(eng.train_step(tok).item()) for _ in range(gen.STEPS)]
    np.testing.assert_allclose(losses, z[name + "/loss"], rtol=1e-2)
    P = eng.export_reference(eng.p)
    sl = eng.export_adafactor_slots()
    after, norms = gen.fixture_case({k: z[k] for k in z.files}, name)
    assert sorted(after) == sorted(list(P) + list(sl))
    # stored rows (every row of the small arrays) by relative L2; the whole array by its norm where the fixture keeps a sample
    worst = {True: [], False: []}
    for k, v in P.items():
        w0 = gen.sample(weights[k])
        err = _rel(gen.sample(v) - w0, after[k] - w0)
        if k in norms:
            err = max(err, abs(np.linalg.norm(v.astype(np.float64) - weights[k]) / norms[k] - 1))
        worst[ar.factored_dims(v.shape) is not None].append((err, k))
    for k, v in sl.items():
        base = k.rsplit("_slot_", 1)[0]
        err = _rel(gen.sample(v), after[k])
        if k in norms:
            err = max(err, abs(np.linalg.norm(v.astype(np.float64)) / norms[k] - 1))
        worst[ar.factored_dims(P[base].shape) is not None].append((err / (1 if k.endswith("_slot_m") else 2), k))
    for f in worst:
        worst[f].sort()
        print(name, "factored" if f else "unfactored", "worst:", worst[f][-4:])
    assert worst[True][-1][0] < 0.12, worst[True][-4:]
    assert worst[False][-1][0] < 0.35, worst[False][-4:]
    # the head's pad columns / pad bias entries bit-unchanged
    V, Vp, d = eng.V, eng.Vp, eng.d
    assert torch.all(eng.view(eng.p, "to_logits/linear_out/kernel")[:, V:] == 0)
    assert torch.all(eng.view(eng.p, "to_logits/linear_out/bias")[V:] == -30000.0)


def _teacher_forced(cfg, B, hp, steps, seed=0):
    """engine steps; each optimizer step checked against the float64 update of the SAME gradient and state"""
    P0 = do.init_params(cfg, seed=1234 + seed, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(B, cfg.text_seq_len, cfg.text_vocab_size, seed=seed + 1),
                                do.synthetic_image_tokens(B, cfg.image_seq_len, cfg.image_vocab_size, seed=seed + 2), cfg.text_vocab_size)
    eng = _engine(cfg, B, hp, P0)
    eng.global_step = 1
    tok = torch.from_numpy(tokens).cuda()
    a = ar.hyper_parameters(hp)
    losses, worst = [], 0.0
    for step in range(steps):
        w = OrderedDict((k, v.astype(np.float64)) for k, v in eng.export_reference(eng.p).items())
        slots = OrderedDict((k, v.astype(np.float64)) for k, v in eng.export_adafactor_slots().items()) if step else None
        losses.append(float(eng.forward(tok, need_grad=True).item()))
        eng.backward()
        eng.wait_grads()
        g = eng.export_reference(eng.g)
        if slots is None:
            slots = ar.init_slots(OrderedDict((k, v.shape) for k, v in w.items()), a["beta1"])
        gc, _ = do.clip_by_global_norm(g, hp["gradient_clipping"])
        lr = eng.optimizer_step()
        assert lr == do.learning_rate(eng.global_step - 1, hp["lr"], hp["train_steps"], hp["warmup_steps"])
        ref = ar.apply_grads(w, gc, slots, lr, **a)
        got, gs = eng.export_reference(eng.p), eng.export_adafactor_slots()
        for k in ref:
            worst = max(worst, _rel(got[k] - w[k], ref[k] - w[k]))
        for k in slots:
            worst = max(worst, _rel(gs[k], slots[k]))
    return eng, P0, tokens, losses, worst


@pytest.mark.parametrize("d,H,L,tv,iv,T,P", [(256, 2, 2, 300, 64, 16, 112), (64, 1, 2, 40, 16, 6, 10)])
def test_engine_against_the_float64_path(d, H, L, tv, iv, T, P):
    """five steps at a width that factors (256) and one that does not (64): each update within 1e-4 of the float64 update of the
    engine's own gradient and state; the loss trajectory within 1e-2 of the float64 path's (bf16 compute vs fp32 oracle)"""
    cfg = do.DalleConfig(d, tv, iv, T, P, L, H)
    hp = dict(optimizer="adafactor", lr=1e-2, train_steps=1000, warmup_steps=2, gradient_clipping=1.0, weight_decay=0.0, beta_1=0.9)
    eng, P0, tokens, losses, worst = _teacher_forced(cfg, 2, hp, 5)
    print("worst update / slot error vs float64:", worst)
    assert worst < 1e-4
    _, _, ref_losses = ar.train(P0, tokens, cfg, hp, 5, 1)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-2)
    assert losses[-1] < losses[0]


CFG_SMALL = dict(d=128, H=1, L=1, tv=150, iv=20, T=8, P=8)


def _small(hp_extra=None, opt="adafactor"):
    c = CFG_SMALL
    cfg = do.DalleConfig(c["d"], c["tv"], c["iv"], c["T"], c["P"], c["L"], c["H"])
    hp = dict(optimizer=opt, lr=1e-2, train_steps=1000, warmup_steps=2, gradient_clipping=1.0, weight_decay=0.1, beta_1=0.9)
    hp.update(hp_extra or {})
    P0 = do.init_params(cfg, seed=5, perturb=0.05)
    tokens = do.assemble_tokens(do.synthetic_captions(2, c["T"], c["tv"], seed=1), do.synthetic_image_tokens(2, c["P"], c["iv"], seed=2), c["tv"])
    return cfg, hp, P0, torch.from_numpy(tokens).cuda()


def _state(eng):
    out = {"p": eng.p.cpu().numpy().view(np.uint32), "slots": eng.af_slots.cpu().numpy().view(np.uint32),
           "pb": eng.pb.view(torch.int16).cpu().numpy()}
    if eng.m is not None:
        out["m"] = eng.m.cpu().numpy().view(np.uint32)
    return out


def test_engine_runs_are_bit_identical():
    cfg, hp, P0, tok = _small()
    runs = []
    for _ in range(2):
        eng = _engine(cfg, 2, hp, P0)
        for _ in range(3):
            eng.train_step(tok)
        runs.append(_state(eng))
        del eng
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_checkpoint_resume_is_bit_identical_and_cross_optimizer_is_refused(tmp_path):
    cfg, hp, P0, tok = _small()
    full = _engine(cfg, 2, hp, P0)
    for _ in range(4):
        full.train_step(tok)
    first = _engine(cfg, 2, hp, P0)
    for _ in range(2):
        first.train_step(tok)
    path = str(tmp_path / "ck.pt")
    torch.save({"dalle": first.state_dict()}, path)
    sd = torch.load(path, map_location="cpu")["dalle"]
    assert sd["optimizer"] == "adafactor" and "v" not in sd and "af_slots" in sd
    resumed = _engine(cfg, 2, hp, do.init_params(cfg, seed=99))
    resumed.load_state_dict(sd)
    assert resumed.global_step == 2
    for _ in range(2):
        resumed.train_step(tok)
    a, b = _state(full), _state(resumed)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # Adam checkpoint into an Adafactor run, and the reverse
    cfg, hpa, P0, tok = _small(opt="adam")
    adam = _engine(cfg, 2, hpa, P0)
    adam.train_step(tok)
    with pytest.raises(ValueError, match="written by the adam optimizer; this run uses adafactor"):
        resumed.load_state_dict(adam.state_dict())
    with pytest.raises(ValueError, match="written by the adafactor optimizer; this run uses adam"):
        adam.load_state_dict(sd)


def test_adafactor_state_is_smaller_than_adam():
    cfg, hp, P0, tok = _small()
    eng = _engine(cfg, 2, hp, P0)
    n = eng.lay.total
    assert eng.v is None and eng.af_slots.numel() < n // 4
    eng2 = _engine(cfg, 2, dict(hp, beta_1=0.0), P0)
    assert eng2.m is None and eng2.v is None


def test_train_dalle_cli_with_adafactor(tmp_path):
    cfg = json.load(open(os.path.join(ROOT, "configs", "dalle_example.json")))
    cfg.update(optimizer="adafactor", n_layers=1, n_embd=256, n_heads=2, train_batch_size=4, eval_batch_size=4, train_steps=6,
               steps_per_checkpoint=6, eval_steps=0, iterations=1, warmup_steps=1, lr=0.01, allow_random_vae=True,
               model_path=str(tmp_path / "run"))
    path = str(tmp_path / "dalle_adafactor.json")
    json.dump(cfg, open(path, "w"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "train_dalle.py"), "--model", path], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=600)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    import re
    losses = [float(x) for x in re.findall(r"step \d+: loss ([0-9.naife+-]+)", out)]
    assert len(losses) >= 3, out[-2000:]
    assert all(math.isfinite(x) for x in losses) and losses[-1] < losses[0], losses
    cks = os.listdir(tmp_path / "run")
    assert any(c.endswith(".pt") for c in cks), cks
    ck = sorted(c for c in cks if c.endswith(".pt"))[-1]
    assert torch.load(str(tmp_path / "run" / ck), map_location="cpu")["dalle"]["optimizer"] == "adafactor"
