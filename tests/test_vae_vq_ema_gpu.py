"""EMA codebook updates and dead-code restarts of the vector-quantised VAE on the GPU: dmi_vq_cluster_sums against int64 / float64
numpy sums (exact on integer-valued rows, inside the any-order fp32 bound on normal ones, two runs equal, unpicked codes exactly 0,
nothing written past the outputs; M below and above the row-chunk size of the kernel), dmi_vq_ema_step against the numpy restatement
of tests/vq_ema_ref.py (N, S, idle, restarts bit for bit, C within one fp32 ulp, the bf16 copy the RNE of the kernel's own C,
unchanged codes untouched in both copies; restarts with pre-aged codes and with two dead codes on one row), and the engine: eager =
captured, the restatement on the engine's own buffers after every step, no codebook gradient or Adam state, loss = recon + beta Lq,
evaluation leaves the state alone, checkpoints, statistics, restarts end to end, the model function."""
import hashlib
import os

import numpy as np
import pytest
import torch

import dalle_hip as dh
import vq_ema_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345
EXTRA = 3
CHUNK = 4096            # rows per chunk of dmi_vq_cluster_sums: above it the partial sums go through the workspace


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).bfloat16()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _cluster_sums(xd, idd, M, T, D, ldx=None):
    """sums [T, D], counts [T] as numpy; checks the sentinels past both ends"""
    sums = torch.full((T + EXTRA, D), float(SENTINEL), dtype=torch.float32, device=DEV)
    counts = torch.full((T + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    nb = dh.vq_cluster_sums_workspace_bytes(M, T, D)
    assert (nb == 0) == (M <= CHUNK)
    ws = torch.full((nb + 64,), 0x5A, dtype=torch.uint8, device=DEV) if nb else None
    dh.vq_cluster_sums(xd, D if ldx is None else ldx, idd, sums, counts, M, T, D, ws)
    torch.cuda.synchronize()
    assert (sums[T:] == SENTINEL).all() and (counts[T:] == SENTINEL).all(), "written past the end"
    if ws is not None:
        assert (ws[nb:] == 0x5A).all(), "workspace written past dmi_vq_cluster_sums_workspace_bytes"
    return sums[:T].cpu().numpy(), counts[:T].cpu().numpy()


def _check_sums(M, T, D, kinds=ref.IDX_KINDS):
    for j, kind in enumerate(kinds):
        idx = ref.make_idx(kind, M, T, seed=j)
        idd = _i32(idx)
        # integer-valued rows: every partial sum is an integer below 2^24, so the sums are exact in any order
        x = ref.make_x(M, D, integer=True, seed=j)
        n64, s64, _ = ref.cluster_sums64(x, idx, T)
        s, n = _cluster_sums(_bf(x), idd, M, T, D)
        assert np.array_equal(n, n64), (kind, "counts")
        assert np.array_equal(s.view(np.uint32), s64.astype(np.float32).view(np.uint32)), (kind, "integer sums differ")
        # normal rows: |s - s64| <= n_k u sum|x| whatever the order; twice the same bits; unpicked codes exactly +0
        x = ref.make_x(M, D, integer=False, seed=j)
        n64, s64, a64 = ref.cluster_sums64(x, idx, T)
        xd = _bf(x)
        s, n = _cluster_sums(xd, idd, M, T, D)
        s2, n2 = _cluster_sums(xd, idd, M, T, D)
        assert np.array_equal(n, n64) and np.array_equal(n2, n64)
        assert np.array_equal(s.view(np.uint32), s2.view(np.uint32)), (kind, "two runs differ")
        err, bound = np.abs(s.astype(np.float64) - s64), n64[:, None] * ref.U * a64
        print(kind, M, T, D, "worst error / bound:", float(np.max(err / np.maximum(bound, 1e-300))), flush=True)
        assert (err <= bound).all(), (kind, float(np.max(err / np.maximum(bound, 1e-300))))
        assert (s.view(np.uint32)[n64 == 0] == 0).all(), (kind, "an unpicked code is not +0")


@pytest.mark.parametrize("M", ref.M_VALUES)
@pytest.mark.parametrize("T", ref.T_VALUES)
@pytest.mark.parametrize("D", ref.D_VALUES)
def test_cluster_sums_vs_numpy(D, T, M):
    _check_sums(M, T, D)


@pytest.mark.parametrize("M", [CHUNK, CHUNK + 1, 9001, 8 * CHUNK + 517])
def test_cluster_sums_across_row_chunks(M):
    """the largest single chunk; the first size with two chunks (whole 512-row rounds each, the last one ragged); three chunks; more
    rows than eight chunks of CHUNK (the number of chunks is capped, they grow instead).  With all rows on one code every chunk
    contributes to the same sum, and the partial sums are added in chunk order"""
    _check_sums(M, 64, 64)


def test_cluster_sums_pitch_and_out_of_range_idx():
    """a row pitch above D; an idx outside [0, T) contributes to nothing"""
    M, T, D, ld = 300, 64, 64, 72
    x = ref.make_x(M, ld, integer=True, seed=9)
    idx = ref.make_idx("uniform", M, T, seed=9)
    bad = idx.copy()
    bad[::5] = np.where(np.arange(M)[::5] % 2 == 0, -1, T + 3)
    keep = (bad >= 0) & (bad < T)
    n64, s64, _ = ref.cluster_sums64(x[keep][:, :D], bad[keep], T)
    s, n = _cluster_sums(_bf(x), _i32(bad), M, T, D, ldx=ld)
    assert np.array_equal(n, n64) and np.array_equal(s, s64.astype(np.float32))


# ------------------------------------------------------------------ dmi_vq_ema_step
def _ema_case(M, T, D, gamma, R, seed, step, idx_kind="uniform", idle=None, use_step_dev=False):
    g = np.random.default_rng(7 + M + T + D)
    x = ref.make_x(M, D, integer=False, seed=3)
    idx = ref.make_idx(idx_kind, M, T, seed=3)
    C = g.standard_normal((T, D)).astype(np.float32)
    Cb_bits = g.integers(0x3C00, 0x4100, (D, T)).astype(np.int16)            # a bf16 copy that is NOT the rounding of C: it must survive
    st = dict(N=(0.25 + 4.0 * g.random(T)).astype(np.float32), S=g.standard_normal((T, D)).astype(np.float32),
              idle=(g.integers(0, 3, T) if idle is None else idle).astype(np.int32), restarts=5)
    xd, idd = _bf(x), _i32(idx)
    s, n = _cluster_sums(xd, idd, M, T, D)
    want_C, want, changed = ref.ema_step(C, st, s, n, x, gamma, R=R, seed=seed, step=step)
    C32 = torch.full((D + EXTRA, T), float(SENTINEL), dtype=torch.float32, device=DEV)
    C32[:D] = _f32(C.T)
    C16 = torch.full((D + EXTRA, T), SENTINEL, dtype=torch.int16, device=DEV)
    C16[:D] = torch.from_numpy(Cb_bits).to(DEV)
    N, S = torch.full((T + 8,), float(SENTINEL), device=DEV), torch.full((T + EXTRA, D), float(SENTINEL), device=DEV)
    N[:T], S[:T] = _f32(st["N"]), _f32(st["S"])
    idl = torch.full((T + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    idl[:T] = _i32(st["idle"])
    rs = torch.tensor([st["restarts"], SENTINEL], dtype=torch.int32, device=DEV)
    step_dev = torch.tensor([step], dtype=torch.int64, device=DEV) if use_step_dev else None
    dh.vq_ema_step(C32, C16.view(torch.bfloat16), N, S, idl, rs[0:1], _f32(s), _i32(n), xd, D, gamma, R, seed,
                   12345 if use_step_dev else step, M, T, D, step_dev=step_dev)     # with step_dev the by-value step is ignored
    torch.cuda.synchronize()
    assert (C32[D:] == SENTINEL).all() and (C16[D:] == SENTINEL).all() and (N[T:] == SENTINEL).all() and (S[T:] == SENTINEL).all()
    assert (idl[T:] == SENTINEL).all() and int(rs[1]) == SENTINEL, "written past the end"
    got_C, got_b = C32[:D].cpu().numpy().T, C16[:D].cpu().numpy().T                  # [T, D]
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)             # noqa: E731
    assert np.array_equal(bits(N[:T].cpu().numpy()), bits(want["N"])), "N"
    assert np.array_equal(bits(S[:T].cpu().numpy()), bits(want["S"])), "S"
    assert np.array_equal(idl[:T].cpu().numpy(), want["idle"]), "idle"
    assert int(rs[0]) == want["restarts"], ("restarts", int(rs[0]), want["restarts"])
    assert (np.abs(got_C.astype(np.float64) - want_C.astype(np.float64)) <= ref.ulp32(want_C)).all(), "C beyond one ulp"
    restarted = changed & (n == 0)
    assert np.array_equal(bits(got_C[restarted]), bits(want_C[restarted])), "a re-seeded code is not its encoder row"
    assert np.array_equal(bits(got_C[~changed]), bits(C[~changed])) and np.array_equal(got_b[~changed], Cb_bits.T[~changed]), "unchanged code touched"
    rne = (ref.round_bf16(got_C[changed]).view(np.uint32) >> 16).astype(np.uint16)
    assert np.array_equal(got_b[changed].view(np.uint16), rne), "bf16 copy is not the RNE of the kernel's C"
    return changed, n, want


@pytest.mark.parametrize("gamma", [0.5, 0.99])
@pytest.mark.parametrize("M", ref.M_VALUES)
@pytest.mark.parametrize("T", ref.T_VALUES)
@pytest.mark.parametrize("D", ref.D_VALUES)
def test_ema_step_vs_restatement(D, T, M, gamma):
    changed, n, want = _ema_case(M, T, D, gamma, R=0, seed=0, step=0)
    assert changed.any() and (not changed.all() or M >= T) and want["restarts"] == 5
    if M == 1030:        # the other idx shapes, once per (D, T)
        for kind in ("one_code", "arange", "top8"):
            _ema_case(M, T, D, gamma, R=0, seed=0, step=0, idx_kind=kind)


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("M,T,D", [(7, 64, 64), (1030, 576, 128), (1030, 4096, 512), (1, 64, 512)])
def test_ema_step_restarts(M, T, D, R):
    """idle counts 0..2 before the step: R = 1 re-seeds every unpicked code, R = 3 only those that were already idle twice; the step
    by value and through the device scalar give the same result (both are compared with the restatement)"""
    for dev in (False, True):
        changed, n, want = _ema_case(M, T, D, 0.9, R=R, seed=17, step=3 + 2 ** 33, use_step_dev=dev)
        assert want["restarts"] > 5 and ((n == 0) & ~changed).any() == (R == 3)


def test_ema_step_two_dead_codes_on_one_row():
    """two dead codes draw the same encoder row: both become that row (the arg-max's tie-break later leaves the higher one idle)"""
    M, T, D = 7, 64, 64
    idx = ref.make_idx("uniform", M, T, seed=3)
    dead = [k for k in range(T) if k not in set(idx.tolist())]
    seed, step = next((s, t) for s in range(50) for t in range(50)
                      if len({ref.restart_row(s, t, k, M) for k in dead[:2]}) == 1)
    changed, n, want = _ema_case(M, T, D, 0.9, R=1, seed=seed, step=step)
    a, b = dead[:2]
    assert ref.restart_row(seed, step, a, M) == ref.restart_row(seed, step, b, M)
    assert changed[a] and changed[b] and np.array_equal(want["S"][a], want["S"][b]) and want["N"][a] == want["N"][b] == 1.0


# ------------------------------------------------------------------ engine
SMALL = dict(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch_size=2)       # the SMALL of tests/test_vae_vq_gpu.py
BETA, GAMMA = 0.25, 0.9


def _sha(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _vae(**kw):
    from src.vae_tf import DiscreteVAE
    vae = DiscreteVAE(use_bf16=True, **SMALL, **kw)
    vae.init_params(seed=4321)
    return vae


def _img(vae, t=0):
    from oracle import vae_oracle as vo
    return torch.from_numpy(vo.synthetic_images(vae.B, vae.H, seed=10 + t))


def _state_sha(vae):
    e = vae.vq_ema
    return [_sha(e[k]) for k in ("N", "S", "idle", "restarts")] + [_sha(vae.p), _sha(vae.pb), _sha(vae.codebook_t), _sha(vae.h)]


def _np_state(vae):
    e = vae.vq_ema
    return dict(N=e["N"].cpu().numpy(), S=e["S"].cpu().numpy(), idle=e["idle"].cpu().numpy(), restarts=int(e["restarts"][0]))


def test_engine_initial_state_and_key_off():
    vae = _vae(quantizer="vq", vq_ema_decay=GAMMA)
    C = vae.view(vae.p, "codebook/codebook").cpu().numpy()        # [D, T]
    st = _np_state(vae)
    assert (st["N"] == 1).all() and np.array_equal(st["S"], C.T) and (st["idle"] == 0).all() and st["restarts"] == 0
    assert vae.vq_restart_after == 0 and vae.vq_ema_decay == GAMMA
    off = _vae(quantizer="vq")
    assert off.vq_ema is None and off.vq_ema_decay is None and "vq_ema" not in off.state_dict() and "vq_codebook" not in off.state_dict()
    off.forward(_img(off), return_recon_loss=True, need_grad=False)
    assert set(off.codebook_stats()) == {"perplexity_hard", "codes_used", "codes_used_frac"}


@pytest.mark.parametrize("R", [0, 2])
def test_engine_steps_are_the_restatement_eager_and_captured(R):
    """three steps: after each, N / S / idle / restarts are the restatement's bits and the codebook master is within one ulp of it, on
    the engine's own x_enc, index and cluster sums (which are inside the any-order bound of the float64 sums); the codebook's slices of
    g, m and v are 0; loss is one rounding of recon + beta Lq; eager and captured steps give equal bits"""
    runs = {}
    for mode in ("eager", "graph"):
        vae = _vae(quantizer="vq", vq_commitment=BETA, vq_ema_decay=GAMMA, vq_restart_after=R or None, vq_restart_seed=3 if R else None)
        D, T, Mg = vae.n_hid, vae.num_tokens, vae.Mg
        out = []
        for t in range(3):
            C0, st0 = vae.view(vae.p, "codebook/codebook").cpu().numpy().T.copy(), _np_state(vae)
            loss = vae.train_step(_img(vae, t), 1e-3, graph=(mode == "graph"))
            torch.cuda.synchronize()
            assert vae.global_step == t + 1
            r, q = np.float64(vae.loss_recon.item()), np.float64(vae.loss_vq.item())
            assert np.float32(loss.item()).tobytes() == np.float32(r + np.float64(np.float32(BETA)) * q).tobytes(), (loss.item(), r, q)
            x, idx = vae.x_enc.float().cpu().numpy(), vae.index.cpu().numpy()
            n64, s64, a64 = ref.cluster_sums64(x, idx, T)
            s, n = vae._ema_sums.cpu().numpy(), vae._ema_counts.cpu().numpy()
            assert np.array_equal(n, n64) and (np.abs(s - s64) <= n64[:, None] * ref.U * a64).all()
            want_C, want, changed = ref.ema_step(C0, st0, s, n, x, GAMMA, R=R, seed=3, step=t)
            st1 = _np_state(vae)
            for k in ("N", "S", "idle"):
                assert np.array_equal(st1[k].view(np.uint32), want[k].view(np.uint32)), (mode, t, k)
            assert st1["restarts"] == want["restarts"]
            got_C = vae.view(vae.p, "codebook/codebook").cpu().numpy().T
            assert (np.abs(got_C.astype(np.float64) - want_C) <= ref.ulp32(want_C)).all() and np.array_equal(got_C[~changed], C0[~changed])
            assert changed.any() and np.array_equal(vae.view(vae.pb, "codebook/codebook").float().cpu().numpy(), ref.round_bf16(got_C.T))
            assert np.array_equal(vae.codebook_t.float().cpu().numpy(), ref.round_bf16(got_C))          # the compute copies followed
            for buf in (vae.g, vae.m, vae.v):
                assert (vae.view(buf, "codebook/codebook") == 0).all()
            assert all(np.abs(vae.view(vae.g, c.name + "/kernel").cpu().numpy()).max() > 0 for c in vae.convs)
            out += [_sha(loss), _sha(vae.index)] + _state_sha(vae)
        if mode == "graph":
            assert len(vae._graphs) == 1
        if R:
            assert _np_state(vae)["restarts"] > 0 or (_np_state(vae)["idle"] < R).all()
        runs[mode] = out + [_sha(vae.g), _sha(vae.m), _sha(vae.v)]
        del vae
    assert runs["eager"] == runs["graph"]


def test_engine_evaluation_leaves_the_state_alone_and_stats():
    vae = _vae(quantizer="vq", vq_ema_decay=GAMMA, vq_restart_after=1)
    for t in range(2):
        vae.train_step(_img(vae, t), 1e-3, graph=False)
    before = _state_sha(vae)
    img = _img(vae, 7)
    vae.forward(img, return_recon_loss=True, need_grad=False)
    vae.mode = "eval"
    loss, _ = vae.forward(img, return_recon_loss=True)
    r, q = np.float64(vae.loss_recon.item()), np.float64(vae.loss_vq.item())
    assert np.float32(loss.item()).tobytes() == np.float32(r + np.float64(np.float32(0.25)) * q).tobytes()
    vae.forward(img, return_logits=True)
    vae.decode_tokens(vae.index.view(vae.B, -1).clone())
    st = vae.codebook_stats()
    torch.cuda.synchronize()
    assert _state_sha(vae) == before
    e = _np_state(vae)
    assert set(st) == {"perplexity_hard", "codes_used", "codes_used_frac", "vq_restarts", "codes_idle"}
    assert st["vq_restarts"] == e["restarts"] and st["codes_idle"] == int((e["idle"] >= 1).sum())


def test_engine_checkpoint_round_trip_continues_bit_identically():
    vae = _vae(quantizer="vq", vq_ema_decay=GAMMA, vq_restart_after=2, vq_restart_seed=5)
    for t in range(2):
        vae.train_step(_img(vae, t), 1e-3, graph=False)
    sd = vae.state_dict()
    assert sd["quantizer"] == "vq" and sd["vq_codebook"] == "ema" and set(sd["vq_ema"]) == {"N", "S", "idle", "restarts"}
    twin = _vae(quantizer="vq", vq_ema_decay=GAMMA, vq_restart_after=2, vq_restart_seed=5)
    twin.load_state_dict(sd)
    assert _state_sha(twin) == _state_sha(vae) and twin.global_step == 2
    for t in (2, 3):
        a, b = vae.train_step(_img(vae, t), 1e-3, graph=False), twin.train_step(_img(twin, t), 1e-3, graph=False)
        assert _sha(a) == _sha(b)
    assert _state_sha(twin) == _state_sha(vae) and _sha(twin.m) == _sha(vae.m) and _sha(twin.v) == _sha(vae.v)
    grad = _vae(quantizer="vq")
    with pytest.raises(ValueError, match="vq_ema_decay"):
        grad.load_state_dict(sd)
    with pytest.raises(ValueError, match="vq_ema_decay"):
        vae.load_state_dict(grad.state_dict())
    # parameters without cluster state (a reference checkpoint): the initial state again
    vae.load_reference_params(vae.export_reference())
    st = _np_state(vae)
    assert (st["N"] == 1).all() and (st["idle"] == 0).all() and st["restarts"] == 0
    assert np.array_equal(st["S"], vae.view(vae.p, "codebook/codebook").cpu().numpy().T)


def test_engine_restarts_revive_dead_codes():
    """lr = 0 and one batch: the encoder does not move.  Half the codes sit at 1e3 and are never picked; R = 1 re-seeds them after the
    first step from encoder rows, which then pick them (a re-seeded code equals an encoder row): more codes in use"""
    vae = _vae(quantizer="vq", vq_ema_decay=GAMMA, vq_restart_after=1, vq_restart_seed=0)
    P = vae.export_reference()
    P["codebook/codebook"][:, vae.num_tokens // 2:] = 1e3
    vae.load_reference_params(P)
    img = _img(vae)
    used, restarts = [], []
    for t in range(3):
        vae.train_step(img, 0.0, graph=False)
        st = vae.codebook_stats()
        used.append(st["codes_used"])
        restarts.append(st["vq_restarts"])
    print("codes used per step:", used, "restarts:", restarts, flush=True)
    assert used[0] <= vae.num_tokens // 2 and restarts[1] > 0
    assert used[2] > used[0]


# ------------------------------------------------------------------ model function
def test_model_fn_with_the_keys(tmp_path, caplog):
    import json
    import logging
    from oracle import vae_oracle as vo
    from src.model_fns_tf import vae_model_fn
    from src.utils import ModeKeys, fetch_model_params
    from src.vae_tf.vq import STAT_SCALARS
    from src.vae_tf.vq_ema import EMA_STAT_SCALARS
    p = fetch_model_params("vae_example")
    p.update(dict(train_batch_size=2, eval_batch_size=2, model_path=str(tmp_path), convblocks=[[1, 64]], num_tokens=64,
                  steps_per_checkpoint=10 ** 6, dataset={"train_path": "synthetic", "eval_path": "synthetic", "image_size": 32},
                  quantizer="vq", vq_commitment=0.5, vq_ema_decay=0.95, vq_restart_after=2, vq_restart_seed=1))
    img = torch.from_numpy(vo.synthetic_images(2, 32, seed=1))
    with caplog.at_level(logging.INFO, logger="dalle_mtf_amd"):
        for _ in range(3):
            spec = vae_model_fn(img, img, ModeKeys.TRAIN, p)
            step = spec.train_op()
            assert np.isfinite(float(spec.loss))
    assert len([r for r in caplog.records if "EMA codebook" in r.getMessage()]) == 1
    fn, tensors = spec.host_call
    fn(step, **tensors)
    rec = json.loads(open(tmp_path / "summaries.jsonl").read().strip().splitlines()[-1])
    assert set(STAT_SCALARS) | set(EMA_STAT_SCALARS) <= set(rec) and rec["step"] == 3, rec
    model = p["_vae_state_train"]["model"]
    assert model.vq_ema_decay == 0.95 and model.vq_restart_after == 2 and model.vq_restart_seed == 1
    ev = vae_model_fn(img, img, ModeKeys.EVAL, p)
    m = ev.eval_metrics
    assert set(m) == {"_loss"} | set(STAT_SCALARS) | set(EMA_STAT_SCALARS)
    assert m["vq_restarts"] >= 0 and 0 <= m["codes_idle"] <= 64
    assert np.float32(float(ev.loss)) == np.float32(np.float64(m["loss_recon"]) + 0.5 * np.float64(m["loss_vq"]))
    with pytest.raises(ValueError, match="vq_ema_decay"):
        bad = p.copy()
        del bad["vq_commitment"]        # it needs "quantizer": "vq" too, and its refusal would come first
        bad.update(_vae_state_train=None, _vae_state_eval=None, quantizer=None)
        vae_model_fn(img, img, ModeKeys.TRAIN, bad)
