"""Vector-quantised bottleneck of the discrete VAE on the GPU: dmi_vq_assign, dmi_vq_half_norms, dmi_vq_scores_bias, dmi_vq_loss,
dmi_vq_bwd_x, dmi_vq_codebook_grad and dmi_vq_gather against the float64 specification of tests/vae_vq_ref.py inside its derived
bounds (D: one, two and eight k-chunks; T: one column tile, a count that is no power of two, the largest; M: a lone row, a ragged
block, several blocks with a ragged last one; five input families), their bit-level contracts (sentinel rows past the end of every
output untouched, two runs equal, beta = 0 copies d, an unpicked code gets exactly 0), and the engine: key off is today's step
launch for launch and bit for bit; with "vq" nothing of size [M, T] is launched, loss / index / gradients are the specification on the
engine's own buffers, graph = eager, tokenising, decoding, checkpoints, codebook_stats() and the model function."""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import dalle_hip as dh
import vae_vq_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345            # as an int16: a bf16 that is never a code or a gradient; as an int32 / float: never an index or a score
EXTRA = 3                    # rows past the end of every output


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV).bfloat16()


def _bits(t):
    return t.contiguous().view(torch.int16).cpu()


def _half_norms(Cd, T, D):
    h = torch.full((T + 8,), float(SENTINEL), dtype=torch.float32, device=DEV)
    dh.vq_half_norms(h, T, D, codebook_t=Cd, ldc=D)
    torch.cuda.synchronize()
    assert (h[T:] == SENTINEL).all(), "h written past the end"
    return h[:T].contiguous()


def _assign(Xd, Cd, h, M, T, D, want_xq=True, want_score=True):
    idx = torch.full((M + EXTRA,), SENTINEL, dtype=torch.int32, device=DEV)
    xq = torch.full((M + EXTRA, D), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    sc = torch.full((M + EXTRA,), float(SENTINEL), dtype=torch.float32, device=DEV)
    dh.vq_assign(Xd, D, Cd, D, h, idx, xq if want_xq else None, D, sc if want_score else None, M, T, D)
    torch.cuda.synchronize()
    assert (idx[M:] == SENTINEL).all() and (_bits(xq[M:]) == SENTINEL).all() and (sc[M:] == SENTINEL).all(), "rows >= M written"
    if not want_xq:
        assert (_bits(xq) == SENTINEL).all(), "a null xq was written"
    if not want_score:
        assert (sc == SENTINEL).all(), "a null score was written"
    return idx[:M], xq[:M], sc[:M]


_SPEC = {}


def _case(fam, M, D, T):
    """inputs and their float64 specification, computed once per case and left unchanged"""
    key = (fam, M, D, T)
    if key not in _SPEC:
        X, C = ref.family(fam, M, D, T)
        _SPEC[key] = (X, C, ref.assign_spec(X, C))
        if len(_SPEC) > 12:
            _SPEC.pop(next(iter(_SPEC)))
    return _SPEC[key]


@pytest.mark.parametrize("M", ref.M_VALUES)
@pytest.mark.parametrize("T", ref.T_VALUES)
@pytest.mark.parametrize("D", ref.D_VALUES)
def test_vq_assign_vs_float64(D, T, M):
    for fam in ref.FAMILIES:
        X, C, sp = _case(fam, M, D, T)
        Xd, Cd = _bf(X), _bf(C)
        h = _half_norms(Cd, T, D)
        herr = np.abs(h.double().cpu().numpy() - sp["h"])
        assert (herr <= ref.h_bound(C)).all(), (fam, D, T, M, "h", float(np.max(herr / ref.h_bound(C))))
        idx, xq, sc = _assign(Xd, Cd, h, M, T, D)
        got = idx.cpu().numpy()
        deficit, undecided, werr = ref.check_assign(sp, got, sc.double().cpu().numpy())
        print(fam, D, T, M, "deficit / bound_m: %.3g  winning score error / (bound_m / 2): %.3g  h error / bound: %.3g  undecided rows: %.4f"
              % (deficit, werr, float(np.max(herr / ref.h_bound(C))), undecided), flush=True)
        if fam in ref.CAPPED:
            assert undecided <= ref.CAP, (fam, D, T, M, undecided)
        if fam == "dup":
            assert (got < T // 2).all(), (fam, D, T, M, "a duplicate column won over its lower twin")
        assert torch.equal(_bits(xq), _bits(Cd[idx.long()])), (fam, D, T, M, "xq is not the gather of the picked codes")
        idx2, xq2, sc2 = _assign(Xd, Cd, h, M, T, D)
        assert torch.equal(idx2, idx) and torch.equal(_bits(xq2), _bits(xq)) and torch.equal(sc2.view(torch.int32), sc.view(torch.int32))
        idx3, _, _ = _assign(Xd, Cd, h, M, T, D, want_xq=False, want_score=False)
        assert torch.equal(idx3, idx)


def test_vq_assign_pitches_and_position_independence():
    """row pitches above D (the padding is never read into a score or written), and a score does not depend on where its row or its
    column sits: the rows in reverse order and the codebook rotated by 64 columns give the same winning scores bit for bit"""
    M, D, T = 200, 128, 576
    X, C = ref.family("normal", M, D, T)
    Xd, Cd = _bf(X), _bf(C)
    h = _half_norms(Cd, T, D)
    idx, xq, sc = _assign(Xd, Cd, h, M, T, D)
    ld = D + 8
    Xp = torch.full((M, ld), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    Cp = torch.full((T, ld), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    Xp[:, :D], Cp[:, :D] = Xd, Cd
    idxp = torch.empty(M, dtype=torch.int32, device=DEV)
    xqp = torch.full((M, ld), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    scp = torch.empty(M, dtype=torch.float32, device=DEV)
    dh.vq_assign(Xp, ld, Cp, ld, h, idxp, xqp, ld, scp, M, T, D)
    assert torch.equal(idxp, idx) and torch.equal(scp.view(torch.int32), sc.view(torch.int32))
    assert torch.equal(_bits(xqp[:, :D]), _bits(xq)) and (_bits(xqp[:, D:]) == SENTINEL).all()
    Xr, Cr = Xd.flip(0).contiguous(), torch.roll(Cd, 64, 0).contiguous()
    hr = _half_norms(Cr, T, D)
    assert torch.equal(hr.view(torch.int32), torch.roll(h, 64, 0).view(torch.int32))
    idxr, _, scr = _assign(Xr, Cr, hr, M, T, D)
    assert torch.equal(scr.flip(0).view(torch.int32), sc.view(torch.int32))
    assert torch.equal((idxr.flip(0) - 64) % T, idx)


def _streaming_case(M, D, T=576):
    X, C, sp = _case("cluster", M, D, T)
    g = np.random.default_rng([M, D, 5])
    idx = sp["idx"].astype(np.int32)
    idx = np.where(g.random(M) < 0.3, g.integers(0, T, size=M), idx).astype(np.int32)      # not every row sits next to its code
    return X, C, idx, ref.bwd_inputs(X, C)


@pytest.mark.parametrize("M", ref.M_VALUES)
@pytest.mark.parametrize("D", ref.D_VALUES)
def test_vq_streaming_kernels_vs_float64(D, M):
    T = 576
    X, C, idx, d = _streaming_case(M, D)
    Xd, Cd, dd, idd = _bf(X), _bf(C), _bf(d), torch.from_numpy(idx).to(DEV)
    # gather
    xq = torch.full((M + EXTRA, D), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    dh.vq_gather(Cd, D, idd, xq, D, M, T, D)
    assert (_bits(xq[M:]) == SENTINEL).all() and torch.equal(_bits(xq[:M]), _bits(Cd[idd.long()]))
    xqn = C[idx]
    # Lq
    ws = torch.empty(int(dh.vq_loss_workspace_bytes()) + 64, dtype=torch.uint8, device=DEV)
    out = torch.full((2,), float(SENTINEL), dtype=torch.float32, device=DEV)
    dh.vq_loss(Xd, D, xq, D, out, M, D, ws)
    lq, want = float(out[0]), ref.lq_spec(X, xqn)
    print(D, M, "Lq error / bound:", abs(lq - want) / ref.lq_bound(X, xqn), flush=True)
    assert out[1] == SENTINEL and abs(lq - want) <= ref.lq_bound(X, xqn), (D, M, lq, want)
    out2 = torch.zeros(2, dtype=torch.float32, device=DEV)
    dh.vq_loss(Xd, D, xq, D, out2, M, D, ws)
    assert np.float32(out2[0].item()).tobytes() == np.float32(lq).tobytes()
    # dX
    for beta in (0.25, 2.0):
        dx = torch.full((M + EXTRA, D), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
        dh.vq_bwd_x(dd, D, Xd, D, xq, D, dx, D, M, D, beta)
        assert (_bits(dx[M:]) == SENTINEL).all(), "rows >= M written"
        want, bound = ref.dx_spec(d, X, xqn, beta)
        err = np.abs(dx[:M].double().cpu().numpy() - want)
        print(D, M, beta, "dX worst error / bound:", float(np.max(err / bound)), flush=True)
        assert (err <= bound).all(), (D, M, beta, float(np.max(err / bound)))
        dx2 = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
        dh.vq_bwd_x(dd, D, Xd, D, xq, D, dx2, D, M, D, beta)
        assert torch.equal(_bits(dx2), _bits(dx[:M]))
    dz = -dd          # holds -0 where d rounds to 0: beta = 0 must hand every bit through
    dx = torch.empty(M, D, dtype=torch.bfloat16, device=DEV)
    dh.vq_bwd_x(dz, D, Xd, D, xq, D, dx, D, M, D, 0.0)
    assert torch.equal(_bits(dx), _bits(dz)), "beta = 0 is not d"
    # dC
    want, bound = ref.dc_spec(X, idx, C)
    dC = _codebook_grad(Xd, idd, Cd, M, T, D)
    got = dC.double().cpu().numpy().T
    err = np.abs(got - want)
    n = np.bincount(idx, minlength=T)
    assert (got[n == 0] == 0).all(), "an unpicked code has a gradient"
    ok = bound > 0
    print(D, M, "dC worst error / bound:", float(np.max(err[ok] / bound[ok])) if ok.any() else 0.0, flush=True)
    assert (err <= bound).all(), (D, M, float(np.max(err[ok] / bound[ok])))
    assert torch.equal(_codebook_grad(Xd, idd, Cd, M, T, D).view(torch.int32), dC.view(torch.int32))


def _codebook_grad(Xd, idd, Cd, M, T, D):
    dC = torch.full((D + EXTRA, T), float(SENTINEL), dtype=torch.float32, device=DEV)
    dh.vq_codebook_grad(Xd, D, idd, Cd, D, dC, M, T, D)
    torch.cuda.synchronize()
    assert (dC[D:] == SENTINEL).all(), "dC written past the end"
    return dC[:D].contiguous()


@pytest.mark.parametrize("D", [64, 512])
def test_vq_codebook_grad_extremes(D):
    """one code takes all rows; every row picks its own code; ids outside [0, T) contribute nothing and read nothing"""
    T, M = 576, 1030
    X, C, _ = _case("normal", M, D, T)
    Xd, Cd = _bf(X), _bf(C)
    for idx in (np.full(M, 77), np.arange(M) % T, np.where(np.arange(M) % 5 == 0, -1, np.where(np.arange(M) % 7 == 0, T, 3))):
        idx = idx.astype(np.int32)
        ok = (idx >= 0) & (idx < T)
        want, bound = ref.dc_spec(X[ok], idx[ok], C)
        want, bound = want * ok.sum() / M, bound * ok.sum() / M          # the scale is 2 / (M D) with the kernel's M
        got = _codebook_grad(Xd, torch.from_numpy(idx).to(DEV), Cd, M, T, D).double().cpu().numpy().T
        n = np.bincount(idx[ok], minlength=T)
        assert (got[n == 0] == 0).all() and (np.abs(got - want) <= bound).all(), (D, idx[:8], float(np.max(np.abs(got - want))))
    out = torch.full((4, D), SENTINEL, dtype=torch.int16, device=DEV).view(torch.bfloat16)
    dh.vq_gather(Cd, D, torch.tensor([0, -1, T, T - 1], dtype=torch.int32, device=DEV), out, D, 4, T, D)
    assert torch.equal(_bits(out[0]), _bits(Cd[0])) and torch.equal(_bits(out[3]), _bits(Cd[T - 1])) and (out[1:3] == 0).all()


@pytest.mark.parametrize("M", ref.M_VALUES)
def test_vq_scores_bias_and_fp32_half_norms(M):
    T, D = 576, 128
    g = np.random.default_rng([M, 3])
    s = g.standard_normal((M, T)).astype(np.float32)
    Cf = (0.1 * g.standard_normal((D, T))).astype(np.float32)        # the masters' layout [D, T]
    h = torch.full((T + 8,), float(SENTINEL), dtype=torch.float32, device=DEV)
    dh.vq_half_norms(h, T, D, codebook_f32=torch.from_numpy(Cf).to(DEV))
    assert (h[T:] == SENTINEL).all()
    err = np.abs(h[:T].double().cpu().numpy() - ref.half_norms(Cf.T))
    assert (err <= ref.h_bound(Cf.T, from_f32=True)).all(), float(np.max(err / ref.h_bound(Cf.T, from_f32=True)))
    sd = torch.full((M + EXTRA, T), float(SENTINEL), dtype=torch.float32, device=DEV)
    sd[:M] = torch.from_numpy(s).to(DEV)
    hh = h[:T].contiguous()
    dh.vq_scores_bias(sd, hh, M, T)
    assert (sd[M:] == SENTINEL).all(), "rows >= M written"
    assert np.array_equal(sd[:M].cpu().numpy(), s - hh.cpu().numpy()[None, :])       # one fp32 subtraction: numpy's bits


# ------------------------------------------------------------------ engine
SMALL = dict(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch_size=2)                     # the smallest VAE the kernels allow
EXAMPLE = dict(num_tokens=512, dimensions=32, convblocks=[[3, 64], [3, 128], [3, 256]], batch_size=1)     # configs/vae_example.json
SHAPES = [pytest.param(SMALL, id="small"), pytest.param(EXAMPLE, id="vae_example")]
BETA = 0.25


def _sha(t):
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def _vae(shape, **kw):
    from src.vae_tf import DiscreteVAE
    vae = DiscreteVAE(use_bf16=True, **shape, **kw)
    vae.init_params(seed=4321)
    return vae


def _batch(vae, t=0):
    from oracle import vae_oracle as vo
    img = torch.from_numpy(vo.synthetic_images(vae.B, vae.H, seed=10 + t))
    u = torch.from_numpy(vo.synthetic_uniforms((vae.B, vae.grid, vae.grid, vae.num_tokens), seed=20 + t))
    return img, u


@pytest.fixture
def recorder():
    """the launch recorder of tools/launch_trace.py in place of the loaded library, for the duration of one test"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from launch_trace import Recorder
    real = dh.lib()
    rec = dh._lib = Recorder(real)
    try:
        yield rec
    finally:
        dh._lib = real


def _sequence(recorder):
    names = {v: k for k, v in recorder.table.items()}
    return [names[i] for i in recorder.sequence]


@pytest.mark.parametrize("shape", SHAPES)
def test_engine_key_off_is_unchanged(shape, recorder):
    """quantizer=None and "gumbel" are the model without the keyword: the same launches with the same arguments, and loss, gradients,
    weights and Adam state after three steps equal bit for bit; no vq launch, no vq buffer"""
    runs = []
    for kw in ({}, dict(quantizer=None), dict(quantizer="gumbel")):
        vae = _vae(shape, **kw)
        assert not vae.vq_on and vae.quantizer == "gumbel" and not hasattr(vae, "h") and vae.gc2 is not None and vae.logits is not None
        assert "quantizer" not in vae.state_dict()
        recorder.reset()
        losses = []
        for t in range(3):
            img, u = _batch(vae, t)
            losses.append(_sha(vae.train_step(img, 1e-3, noise=u, graph=False)))
        seq = _sequence(recorder)
        assert not any("vq" in c for c in seq)
        runs.append((seq, losses, _sha(vae.g), _sha(vae.p), _sha(vae.m), _sha(vae.v)))
        del vae
    assert runs[0][0] == runs[1][0] == runs[2][0], "launch sequence differs"
    assert runs[0][1:] == runs[1][1:] == runs[2][1:]


@pytest.mark.parametrize("shape", SHAPES)
def test_engine_vq_step_launches_nothing_of_size_m_t(shape, recorder):
    """with "vq" the train step runs no Gumbel, KL or usage launch and no product or element-wise launch over [M, T]: the six
    bottleneck launches of the Gumbel step (logits, y C^T, two codebook gradients, dy, dx_enc) are gone; the [M, T] buffers do not exist"""
    vae = _vae(shape, quantizer="vq")
    assert vae.logits is None and vae.u is None and vae.y is None and vae.y_soft is None and vae.dy is None and vae.dlogits is None
    assert vae.gc2 is None
    recorder.reset()
    img, _ = _batch(vae)
    vae.train_step(img, 1e-3, graph=False)
    seq = _sequence(recorder)
    assert not any(w in c for c in seq for w in ("gumbel", "codebook_kl", "codebook_usage", "add_f32", "scores_bias")), seq
    for name in ("vq_assign", "vq_loss", "vq_bwd_x", "vq_codebook_grad", "vq_half_norms", "elbo_loss"):
        assert sum(c.startswith(name + "(") for c in seq) == 1, (name, seq)
    T, Mg = str(vae.num_tokens), str(vae.Mg)
    for c in seq:          # a GEMM names its sizes: none has both M = Mg rows and the codebook's T among them (SMALL: T = 64 = n_hid)
        if c.startswith(("gemm_nt(", "gemm_tn(")) and shape is EXAMPLE:
            args = c[c.index("(") + 1:-1].split(",")
            assert not (Mg in [a.strip() for a in args] and T in [a.strip() for a in args]), c
    ref_vae = _vae(shape)
    recorder.reset()
    img, u = _batch(ref_vae)
    ref_vae.train_step(img, 1e-3, noise=u, graph=False)
    gemms = lambda s: sum(c.startswith(("gemm_nt(", "gemm_tn(")) for c in s)
    assert gemms(_sequence(recorder)) - gemms(seq) == 6


@pytest.mark.parametrize("recompute", [False, True], ids=["keep", "recompute"])
@pytest.mark.parametrize("shape", SHAPES)
def test_engine_vq_against_float64_on_its_own_buffers(shape, recompute):
    """loss is one fp32 rounding of loss_recon + (1 + beta) loss_vq; idx / xq / loss_vq are the specification on the engine's own x_enc
    and codebook; dX and the codebook gradient are the specification on the engine's own d, x_enc and idx (everything up- and
    downstream is existing, tested code) -- in train and in eval mode, with and without recompute_grad"""
    vae = _vae(shape, quantizer="vq", vq_commitment=BETA, recompute_grad=recompute)
    img, u = _batch(vae)
    D, T, Mg = vae.n_hid, vae.num_tokens, vae.Mg
    for mode in ("train", "eval"):
        vae.mode = mode
        loss, _ = vae.forward(img, return_recon_loss=True, hard_gumbel=(mode == "train"), temperature=0.5, noise=u)      # accepted and ignored
        r, q = np.float64(vae.loss_recon.item()), np.float64(vae.loss_vq.item())
        assert np.float32(loss.item()).tobytes() == np.float32(r + np.float64(np.float32(1.0 + BETA)) * q).tobytes(), (mode, loss.item(), r, q)
        X, C = vae.x_enc.float().cpu().numpy(), vae.codebook_t.float().cpu().numpy()
        assert np.array_equal(C, vae.view(vae.pb, "codebook/codebook").float().cpu().numpy().T)
        sp = ref.assign_spec(X, C)
        idx = vae.index.cpu().numpy()
        print(shape["num_tokens"], mode, "deficit / bound, undecided:", ref.check_assign(sp, idx)[:2], flush=True)
        assert np.array_equal(vae.xdec.float().cpu().numpy(), C[idx])
        herr = np.abs(vae.h.double().cpu().numpy() - sp["h"])
        assert (herr <= ref.h_bound(C)).all()
        assert abs(q - ref.lq_spec(X, C[idx])) <= ref.lq_bound(X, C[idx]) and q > 0 and r > 0
    vae.mode = "train"
    vae.forward(img, return_recon_loss=True, need_grad=True)
    # backward() hands the bottleneck the decoder's gradient in one scratch buffer and writes dX into another: note both as they pass
    seen = {}
    real = dh.vq_bwd_x

    def spy(d, ldd, x, ldx, xq, ldq, dx, lddx, M, Dn, beta):
        seen["d"] = d.reshape(-1)[:M * Dn].view(M, Dn).float().cpu().numpy()
        real(d, ldd, x, ldx, xq, ldq, dx, lddx, M, Dn, beta)
        seen["dx"] = dx.reshape(-1)[:M * Dn].view(M, Dn).double().cpu().numpy()
        seen["beta"] = beta
    dh.vq_bwd_x = spy
    try:
        vae.backward()
    finally:
        dh.vq_bwd_x = real
    torch.cuda.synchronize()
    X, C, idx = vae.x_enc.float().cpu().numpy(), vae.codebook_t.float().cpu().numpy(), vae.index.cpu().numpy()
    assert seen["beta"] == BETA and np.abs(seen["d"]).max() > 0
    want, bound = ref.dx_spec(seen["d"], X, C[idx], BETA)
    err = np.abs(seen["dx"] - want)
    assert (err <= bound).all(), float(np.max(err / bound))
    want, bound = ref.dc_spec(X, idx, C)
    got = vae.view(vae.g, "codebook/codebook").double().cpu().numpy().T
    assert (np.abs(got - want) <= bound).all() and (got[np.bincount(idx, minlength=T) == 0] == 0).all()
    assert np.abs(got).max() > 0 and all(np.abs(vae.view(vae.g, c.name + "/kernel").cpu().numpy()).max() > 0 for c in vae.convs)


@pytest.mark.parametrize("shape", SHAPES)
def test_engine_vq_graph_equals_eager(shape):
    runs = {}
    for mode in ("eager", "graph"):
        vae = _vae(shape, quantizer="vq")
        out = []
        for t in range(3):
            img, _ = _batch(vae, t)
            loss = vae.train_step(img, 1e-3, hard_gumbel=bool(t & 1), temperature=1.0 - 0.2 * t, graph=(mode == "graph"))
            out += [_sha(loss), _sha(vae.loss_recon), _sha(vae.loss_vq), _sha(vae.index)]
        if mode == "graph":
            assert len(vae._graphs) == 1
        runs[mode] = out + [_sha(vae.g), _sha(vae.p), _sha(vae.m), _sha(vae.v), _sha(vae.h)]
        del vae
    assert runs["eager"] == runs["graph"]
    assert len(set(runs["eager"][0:12:4])) == 3         # the steps did differ


@pytest.mark.parametrize("shape", SHAPES)
def test_engine_vq_tokenising_and_decoding(shape):
    vae = _vae(shape, quantizer="vq")
    for t in range(2):                                   # two trained steps: the codebook has moved, h has followed it
        vae.train_step(_batch(vae, t)[0], 1e-2, graph=False)
    vae.mode = "eval"
    img, _ = _batch(vae, 5)
    _, recon = vae.forward(img, return_recon_loss=True, need_grad=False)
    idx = vae.index.clone()
    D, T, Mg = vae.n_hid, vae.num_tokens, vae.Mg
    X, C = vae.x_enc.float().cpu().numpy(), vae.codebook_t.float().cpu().numpy()
    sp = ref.assign_spec(X, C)
    # bf16 path: the scores' arg-max is the training forward's code on every decided row, and the scores are within the bound
    s = vae.forward(img, return_logits=True)
    assert s.shape == (vae.B, vae.grid, vae.grid, T) and s.dtype == torch.float32
    s = s.reshape(Mg, T)
    dec = torch.from_numpy(sp["decided"]).to(DEV)
    assert torch.equal(s.argmax(-1)[dec].int(), idx[dec]) and int(dec.sum()) > 0
    ref.check_assign(sp, s.argmax(-1).cpu().numpy())
    assert (np.abs(s.double().cpu().numpy() - sp["s"]) <= sp["bound"][:, None] / 2).all()
    # decoding: the same reconstruction bit for bit
    out = vae.decode_tokens(idx.view(vae.B, -1))
    assert torch.equal(out, recon)
    # fp32 path: scores of the fp32 masters on the fp32 encoder's output
    vae.fp32_tokens = True
    s32 = vae.forward(img, return_logits=True).reshape(Mg, T).double().cpu().numpy()
    vae.fp32_tokens = False
    Cf = vae.view(vae.p, "codebook/codebook").double().cpu().numpy().T          # [T, D]
    Xf = vae.x_enc_f32[:Mg * D].view(Mg, D).double().cpu().numpy()             # the fp32 encoder's output, as that path left it
    spf = ref.assign_spec(Xf, Cf, products_exact=False)
    err = np.abs(s32 - spf["s"])
    print(shape["num_tokens"], "fp32 scores worst error / (bound_m / 2):", float(np.max(err / (spf["bound"][:, None] / 2))), flush=True)
    assert (err <= spf["bound"][:, None] / 2).all()


@pytest.mark.parametrize("shape", SHAPES)
def test_engine_vq_checkpoints_and_stats(shape, recorder):
    vae = _vae(shape, quantizer="vq")
    for t in range(2):
        vae.train_step(_batch(vae, t)[0], 1e-2)
    assert not any("usage" in c for c in _sequence(recorder))
    sd = vae.state_dict()
    assert sd["quantizer"] == "vq"
    twin = _vae(shape, quantizer="vq", vq_commitment=1.0)
    twin.load_state_dict(sd)
    assert _sha(twin.p) == _sha(vae.p) and _sha(twin.m) == _sha(vae.m) and _sha(twin.h) == _sha(vae.h) and twin.global_step == 2
    gum = _vae(shape)
    with pytest.raises(ValueError, match="quantizer"):
        gum.load_state_dict(sd)
    with pytest.raises(ValueError, match="quantizer"):
        vae.load_state_dict(gum.state_dict())
    vae.mode = "eval"
    vae.forward(_batch(vae, 9)[0], return_recon_loss=True, need_grad=False)
    recorder.reset()
    st = vae.codebook_stats()
    assert [c.split("(")[0] for c in _sequence(recorder)] == ["codebook_usage"]
    assert set(st) == {"perplexity_hard", "codes_used", "codes_used_frac"}
    n = np.bincount(vae.index.cpu().numpy(), minlength=vae.num_tokens)
    p = n[n > 0] / n.sum()
    assert st["codes_used"] == int((n > 0).sum()) and st["codes_used_frac"] == st["codes_used"] / vae.num_tokens
    assert st["perplexity_hard"] == pytest.approx(float(np.exp(-(p * np.log(p)).sum())), rel=1e-12)
    assert vae.codebook_stats() == st


# ------------------------------------------------------------------ model function
def _params(tmp_path, **over):
    from src.utils import fetch_model_params
    p = fetch_model_params("vae_example")
    p.update(dict(train_batch_size=2, eval_batch_size=2, model_path=str(tmp_path), convblocks=[[1, 64]], num_tokens=64,
                  steps_per_checkpoint=10 ** 6, dataset={"train_path": "synthetic", "eval_path": "synthetic", "image_size": 32}))
    p.update(over)
    return p


def test_model_fn_with_the_key(tmp_path, caplog):
    import json
    import logging
    from oracle import vae_oracle as vo
    from src.model_fns_tf import vae_model_fn
    from src.utils import ModeKeys
    from src.vae_tf.vq import STAT_SCALARS
    p = _params(tmp_path, quantizer="vq", vq_commitment=0.5)
    img = torch.from_numpy(vo.synthetic_images(2, 32, seed=1))
    with caplog.at_level(logging.INFO, logger="dalle_mtf_amd"):
        for _ in range(3):
            spec = vae_model_fn(img, img, ModeKeys.TRAIN, p)
            step = spec.train_op()
            assert np.isfinite(float(spec.loss))
    assert len([r for r in caplog.records if "vector quantisation" in r.getMessage()]) == 1
    fn, tensors = spec.host_call
    fn(step, **tensors)
    rec = json.loads(open(tmp_path / "summaries.jsonl").read().strip().splitlines()[-1])
    assert set(STAT_SCALARS) <= set(rec) and "temperature" in rec and "loss" in rec and rec["step"] == 3, rec
    assert not ({"loss_kl", "perplexity_soft", "kl_weight"} & set(rec))
    model = p["_vae_state_train"]["model"]
    assert model.vq_on and model.vq_beta == 0.5
    ev = vae_model_fn(img, img, ModeKeys.EVAL, p)
    m = ev.eval_metrics
    assert set(m) == {"_loss"} | set(STAT_SCALARS) and np.isfinite(float(ev.loss))
    assert 1.0 <= m["perplexity_hard"] <= 64.0 and 0.0 < m["codes_used_frac"] <= 1.0 and m["loss_vq"] > 0 and m["loss_recon"] > 0
    assert np.float32(float(ev.loss)) == np.float32(np.float64(m["loss_recon"]) + 1.5 * np.float64(m["loss_vq"]))


def test_load_vae_model_passes_the_quantizer_through(tmp_path):
    """DALL-E tokenises and decodes with the quantiser the VAE was trained with; a .pt checkpoint of the other one is refused"""
    from src.model_fns import initialize_vae_weights, load_vae_model
    vp = dict(num_tokens=64, convblocks=[[1, 64]], model_path=str(tmp_path), quantizer="vq")
    params = dict(vae_params=vp, dataset=dict(image_size=32), train_batch_size=2, allow_random_vae=True)
    vae, ck = load_vae_model(params, "train")
    assert vae.vq_on and ck is None
    gum = _vae(SMALL)
    path = os.path.join(str(tmp_path), "gumbel.pt")
    torch.save(gum.state_dict(), path)
    with pytest.raises(ValueError, match="quantizer"):
        initialize_vae_weights(vae, path)
    src = _vae(SMALL, quantizer="vq")
    path = os.path.join(str(tmp_path), "vq.pt")
    torch.save(src.state_dict(), path)
    initialize_vae_weights(vae, path)
    assert _sha(vae.p) == _sha(src.p) and _sha(vae.h) == _sha(src.h)
