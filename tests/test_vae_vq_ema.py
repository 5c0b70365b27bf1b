"""EMA codebook updates and dead-code restarts of the vector-quantised VAE, CPU side: the config-key resolver and its log line; the
constructor refuses before any device work; properties of the numpy restatement (tests/vq_ema_ref.py) that the GPU tests compare the
kernels with; the C ABI (declared, exported, bound; argument errors come back as a status and a message before anything is launched
-- the pointers below are never dereferenced); the state-dict rule on a stand-in; the compile-time resources."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dalle-mtf_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import dalle_hip as dh  # noqa: E402
import vq_ema_ref as ref  # noqa: E402
from src.vae_tf.vq import STAT_SCALARS, resolve_vq_options  # noqa: E402
from src.vae_tf.vq_ema import (EMA_STAT_SCALARS, OFF, check_checkpoint, resolve_vq_ema_options, vq_ema_log_lines)  # noqa: E402

FAKE = ctypes.c_void_p(0x10000)
ODD = ctypes.c_void_p(0x10004)
DMI_OK, DMI_ERR_INVALID, DMI_ERR_UNSUPPORTED = 0, -1, -3
SMALL = dict(num_tokens=64, dimensions=32, convblocks=[[1, 64]], batch_size=2)
VQ = dict(quantizer="vq")


# ------------------------------------------------------------------ config keys
def test_resolver_accepts_and_off_means_off():
    assert OFF == (None, 0, 0)
    for p in (None, {}, dict(vq_ema_decay=None), dict(vq_ema_decay=None, vq_restart_after=None, vq_restart_seed=None),
              dict(vq_restart_after=0), dict(VQ, vq_restart_after=0), dict(quantizer="gumbel", vq_restart_after=None)):
        assert resolve_vq_ema_options(p) == OFF, p
    assert resolve_vq_ema_options(dict(VQ, vq_ema_decay=0.99)) == (0.99, 0, 0)
    assert resolve_vq_ema_options(dict(VQ, vq_ema_decay=np.float32(0.5), vq_restart_after=0)) == (0.5, 0, 0)
    assert resolve_vq_ema_options(dict(VQ, vq_ema_decay=0.9, vq_restart_after=None)) == (0.9, 0, 0)
    assert resolve_vq_ema_options(dict(VQ, vq_ema_decay=0.9, vq_restart_after=3)) == (0.9, 3, 0)
    assert resolve_vq_ema_options(dict(VQ, vq_ema_decay=0.9, vq_restart_after=np.int64(1), vq_restart_seed=-7)) == (0.9, 1, -7)
    assert resolve_vq_ema_options(dict(VQ, vq_ema_decay=0.9, vq_commitment=0.5, codebook_stats=True), world=1) == (0.9, 0, 0)
    from collections import defaultdict
    d = defaultdict(lambda: None, quantizer="vq", vq_ema_decay=0.75)         # the shape fetch_model_params returns
    assert resolve_vq_ema_options(d) == (0.75, 0, 0)
    # the quantiser's own options stay a two-field tuple
    assert resolve_vq_options(dict(VQ, vq_ema_decay=0.9)) == ("vq", 0.25)


EMA = dict(VQ, vq_ema_decay=0.9)


@pytest.mark.parametrize("key,value,other", [
    ("vq_ema_decay", 0, VQ), ("vq_ema_decay", 0.0, VQ), ("vq_ema_decay", 1, VQ), ("vq_ema_decay", 1.0, VQ), ("vq_ema_decay", -0.5, VQ),
    ("vq_ema_decay", 1.5, VQ), ("vq_ema_decay", float("nan"), VQ), ("vq_ema_decay", float("inf"), VQ), ("vq_ema_decay", "0.9", VQ),
    ("vq_ema_decay", True, VQ), ("vq_ema_decay", [0.9], VQ),
    ("vq_ema_decay", 0.9, {}), ("vq_ema_decay", 0.9, dict(quantizer="gumbel")), ("vq_ema_decay", 0.9, dict(quantizer=None)),
    ("vq_restart_after", -1, EMA), ("vq_restart_after", 1.0, EMA), ("vq_restart_after", 2.5, EMA), ("vq_restart_after", True, EMA),
    ("vq_restart_after", False, EMA), ("vq_restart_after", "3", EMA), ("vq_restart_after", [3], EMA),
    ("vq_restart_after", 3, VQ), ("vq_restart_after", 3, {}), ("vq_restart_after", 3, dict(VQ, vq_ema_decay=None)),
    ("vq_restart_seed", 1.5, dict(EMA, vq_restart_after=2)), ("vq_restart_seed", True, dict(EMA, vq_restart_after=2)),
    ("vq_restart_seed", "7", dict(EMA, vq_restart_after=2)),
    ("vq_restart_seed", 7, EMA), ("vq_restart_seed", 7, dict(EMA, vq_restart_after=0)), ("vq_restart_seed", 0, VQ),
    ("vq_restart_seed", 7, {}),
])
def test_resolver_refuses_naming_the_key(key, value, other):
    with pytest.raises(ValueError, match=key):
        resolve_vq_ema_options(dict(other, **{key: value}))


def test_resolver_refuses_data_parallel():
    with pytest.raises(ValueError, match="vq_ema_decay.*data-parallel"):
        resolve_vq_ema_options(EMA, world=2)
    assert resolve_vq_ema_options(VQ, world=8) == OFF                 # gradient VQ stays data-parallel


def test_constructor_refuses_before_any_device_work():
    from src.vae_tf import DiscreteVAE
    with pytest.raises(ValueError, match="vq_ema_decay"):
        DiscreteVAE(vq_ema_decay=0.9, **SMALL)
    with pytest.raises(ValueError, match="vq_ema_decay"):
        DiscreteVAE(quantizer="vq", vq_ema_decay=1.0, **SMALL)
    with pytest.raises(ValueError, match="vq_ema_decay"):
        DiscreteVAE(quantizer="vq", vq_ema_decay=0.9, world_size=2, **SMALL)
    with pytest.raises(ValueError, match="vq_restart_after"):
        DiscreteVAE(quantizer="vq", vq_restart_after=2, **SMALL)
    with pytest.raises(ValueError, match="vq_restart_after"):
        DiscreteVAE(quantizer="vq", vq_ema_decay=0.9, vq_restart_after=True, **SMALL)
    with pytest.raises(ValueError, match="vq_restart_seed"):
        DiscreteVAE(quantizer="vq", vq_ema_decay=0.9, vq_restart_seed=3, **SMALL)


def test_log_line_says_what_is_on():
    assert vq_ema_log_lines(OFF, 2048) == [] and vq_ema_log_lines(resolve_vq_ema_options(VQ), 2048) == []
    (line,) = vq_ema_log_lines(resolve_vq_ema_options(dict(EMA, vq_restart_after=4, vq_restart_seed=11)), 2048)
    assert "EMA codebook" in line and "0.9" in line and "2048" in line and "4 steps" in line and "11" in line
    assert all(k in line for k in EMA_STAT_SCALARS)
    (line,) = vq_ema_log_lines(resolve_vq_ema_options(EMA), 512)
    assert "no restarts" in line
    assert STAT_SCALARS == ("loss_recon", "loss_vq", "perplexity_hard", "codes_used_frac")      # the gradient-VQ metric set is as it was


# ------------------------------------------------------------------ the restatement
def test_splitmix_and_restart_row_by_hand():
    # splitmix64(0), written out: z = 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
    # z ^ z >> 31 = 0xE220A8397B1DCDAF (the first output of the published generator seeded with 0)
    assert ref.splitmix64(0) == 0xE220A8397B1DCDAF
    z = 0x9E3779B97F4A7C15
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) % 2 ** 64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) % 2 ** 64
    assert z ^ (z >> 31) == 0xE220A8397B1DCDAF
    # the two-stage hash, stage by stage: seed 0, step 5, code 3, M = 1030
    r = ref.splitmix64(0xE220A8397B1DCDAF ^ 5)
    assert ref.restart_row(0, 5, 3, 1030) == ref.splitmix64((r + 3) % 2 ** 64) % 1030
    assert 0 <= ref.restart_row(0, 5, 3, 1030) < 1030 and ref.restart_row(0, 5, 3, 1) == 0
    assert ref.restart_row(-1, 0, 0, 97) == ref.restart_row(2 ** 64 - 1, 0, 0, 97)      # a negative seed is its 64-bit pattern
    rows = {ref.restart_row(0, s, k, 1030) for s in range(4) for k in range(4)}
    assert len(rows) >= 14                                                           # step and code both move the draw


def _state(T=16, D=8, seed=0):
    g = np.random.default_rng(seed)
    C = g.standard_normal((T, D)).astype(np.float32)
    return C, ref.initial_state(C)


def test_unpicked_code_keeps_its_code_and_its_mean():
    C, st = _state()
    x = ref.make_x(40, 8, integer=False)
    idx = (np.arange(40) % 8).astype(np.int32)           # codes 8..15 are never picked
    n, s, _ = ref.cluster_sums64(x, idx, 16)
    C1, st1 = C, st
    for step in range(25):
        C1, st1, changed = ref.ema_step(C1, st1, s.astype(np.float32), n, x, 0.9, step=step)
        assert not changed[8:].any() and changed[:8].all()
    assert np.array_equal(C1[8:], C[8:])                                        # bit for bit
    assert (st1["idle"][8:] == 25).all() and (st1["idle"][:8] == 0).all() and st1["restarts"] == 0
    assert np.allclose(st1["N"][8:], 0.9 ** 25, rtol=1e-5)
    ratio = st1["S"][8:].astype(np.float64) / st1["N"][8:, None]
    assert np.allclose(ratio, C[8:], rtol=25 * 4 * 2.0 ** -24, atol=0)          # S'/N' = S/N up to the roundings of 25 steps
    assert st["idle"].sum() == 0 and np.array_equal(st["S"], C)                 # inputs untouched


@pytest.mark.parametrize("gamma", [0.5, 0.9])
def test_constant_input_converges_to_it(gamma):
    C, st = _state(T=8, D=8, seed=3)
    row = np.arange(8, dtype=np.float32) - 3.5
    x = np.tile(row, (6, 1))
    idx = np.full(6, 2, np.int32)
    n, s, _ = ref.cluster_sums64(x, idx, 8)
    steps = 40 if gamma == 0.5 else 200
    for step in range(steps):
        C, st, _ = ref.ema_step(C, st, s.astype(np.float32), n, x, gamma, step=step)
    assert np.allclose(C[2], row, rtol=1e-5, atol=1e-6)
    assert np.isclose(st["N"][2], 6.0, rtol=1e-5)


def test_restart_takes_an_encoder_row_and_resets_the_state():
    C, st = _state()
    x = ref.make_x(40, 8, integer=False, seed=1)
    idx = (np.arange(40) % 8).astype(np.int32)
    n, s, _ = ref.cluster_sums64(x, idx, 16)
    st["idle"][12] = 2                                     # pre-aged: restarts at R = 3 in this step; the others only reach 1
    C1, st1, changed = ref.ema_step(C, st, s.astype(np.float32), n, x, 0.9, R=3, seed=5, step=7)
    m = ref.restart_row(5, 7, 12, 40)
    assert np.array_equal(C1[12], x[m]) and np.array_equal(st1["S"][12], x[m]) and st1["N"][12] == 1 and st1["idle"][12] == 0
    assert st1["restarts"] == 1 and changed[12] and not changed[8:12].any() and not changed[13:].any()
    assert (st1["idle"][[8, 9, 10, 11, 13, 14, 15]] == 1).all()
    _, st0, _ = ref.ema_step(C, st, s.astype(np.float32), n, x, 0.9, R=0, seed=5, step=7)
    assert st0["restarts"] == 0 and st0["idle"][12] == 3                      # R = 0 never restarts


def test_round_bf16_ties_to_even():
    a = np.array([1.0, 1.00390625, 1.01171875, -1.00390625, 3.0e38], np.float32)          # 1 + 2^-8 is a tie, 1 + 3 * 2^-8 is a tie
    assert np.array_equal(ref.round_bf16(a)[:4], np.array([1.0, 1.0, 1.015625, -1.0], np.float32))


# ------------------------------------------------------------------ the state-dict rule (host code)
def test_checkpoint_rule():
    check_checkpoint(None, {"vae_variables": {}})
    check_checkpoint(None, {"quantizer": "vq"})
    check_checkpoint(0.9, {"quantizer": "vq", "vq_codebook": "ema"})
    with pytest.raises(ValueError, match="vq_ema_decay"):
        check_checkpoint(None, {"quantizer": "vq", "vq_codebook": "ema"})
    with pytest.raises(ValueError, match="vq_ema_decay"):
        check_checkpoint(0.9, {"quantizer": "vq"})


def _stub(ema):
    import torch

    class Stub:
        global_step, loaded = 3, None
        m = v = torch.zeros(4)
        quantizer, vq_on = "vq", True

        def export_reference(self):
            return {"codebook/codebook": np.zeros((2, 2), np.float32)}

        def load_reference_params(self, P):
            self.loaded = P
    s = Stub()
    if ema:
        s.vq_ema_decay = 0.9
        s.vq_ema = dict(N=torch.tensor([1.5, 0.25]), S=torch.arange(4.0).view(2, 2), idle=torch.tensor([0, 4], dtype=torch.int32),
                        restarts=torch.tensor([6], dtype=torch.int32))
    return s


def test_state_dict_round_trips_and_refuses_the_other_kind():
    import torch
    from src.vae_tf.models import DiscreteVAE
    plain = _stub(False)                                    # the stand-in of tests/test_vae_vq.py: none of the new attributes
    sd_plain = DiscreteVAE.state_dict(plain)
    assert "vq_codebook" not in sd_plain and "vq_ema" not in sd_plain and sd_plain["quantizer"] == "vq"
    DiscreteVAE.load_state_dict(plain, sd_plain)
    assert plain.loaded is not None
    src = _stub(True)
    sd = DiscreteVAE.state_dict(src)
    assert sd["vq_codebook"] == "ema" and set(sd["vq_ema"]) == {"N", "S", "idle", "restarts"}
    dst = _stub(True)
    for t in dst.vq_ema.values():
        t.zero_()
    DiscreteVAE.load_state_dict(dst, sd)
    assert dst.loaded is not None and all(torch.equal(dst.vq_ema[k], src.vq_ema[k]) for k in src.vq_ema)
    assert dst.vq_ema["idle"].dtype == torch.int32
    for model, ck in ((_stub(False), sd), (_stub(True), sd_plain)):
        with pytest.raises(ValueError, match="vq_ema_decay"):
            DiscreteVAE.load_state_dict(model, ck)
        assert model.loaded is None


# ------------------------------------------------------------------ C ABI
SYMBOLS = dict(dmi_vq_cluster_sums_workspace_bytes=3, dmi_vq_cluster_sums=10, dmi_vq_ema_step=19)


def _msg():
    return dh.lib().dmi_last_error_string().decode()


def test_entry_points_are_declared_exported_and_bound():
    L = dh.lib()
    declared = dh.declared_symbols()
    for name, nargs in SYMBOLS.items():
        assert name in declared, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == nargs, name
        assert fn.restype is (ctypes.c_int64 if name.endswith("_bytes") else ctypes.c_int), name
        assert callable(getattr(dh, name[4:]))
    ws = L.dmi_vq_cluster_sums_workspace_bytes
    assert ws(1030, 4096, 512) == 0 and ws(4096, 2048, 512) == 0                      # one chunk of rows: no workspace
    assert ws(16384, 2048, 512) >= 2 * 2048 * 513 * 4 and ws(16384, 2048, 512) % 16 == 0
    assert ws(1 << 31, 4096, 512) == ws(1 << 20, 4096, 512) <= 8 * 4096 * 513 * 4      # the number of chunks is capped
    # the existing entry points keep their argument counts
    assert len(L.dmi_vq_codebook_grad.argtypes) == 11 and len(L.dmi_elbo_loss.argtypes) == 6 and len(L.dmi_vq_assign.argtypes) == 13


def _sums(M=8, T=64, D=64, ld=None, x=FAKE, idx=FAKE, sums=FAKE, counts=FAKE, ws=None):
    return dh.lib().dmi_vq_cluster_sums(x, D if ld is None else ld, idx, sums, counts, M, T, D, ws, None)


def test_cluster_sums_argument_errors():
    for kw, word in ((dict(M=0), "M must be positive"), (dict(M=-3), "M must be positive"), (dict(x=None), "null"), (dict(idx=None), "null"),
                     (dict(sums=None), "null"), (dict(counts=None), "null"), (dict(ld=60), "ldx"), (dict(ld=32), "ldx"), (dict(D=0), "positive"),
                     (dict(T=0), "positive"), (dict(x=ODD), "aligned"), (dict(idx=ODD), "aligned"), (dict(sums=ODD), "aligned"),
                     (dict(ws=ODD), "aligned"), (dict(M=4097), "workspace")):
        assert _sums(**kw) == DMI_ERR_INVALID and _msg().startswith("vq_cluster_sums") and word in _msg(), (kw, _msg())
    for kw in (dict(D=12, ld=16), dict(D=520), dict(D=1024), dict(T=12), dict(T=4104), dict(T=8192)):
        assert _sums(**kw) == DMI_ERR_UNSUPPORTED and _msg().startswith("vq_cluster_sums"), (kw, _msg())
        with pytest.raises(dh.DalleHipError):
            dh._check(_sums(**kw), "vq_cluster_sums")


def _ema(M=8, T=64, D=64, ld=None, gamma=0.9, R=0, seed=0, step=0, step_dev=None, **ptr):
    names = ("codebook_f32", "codebook_bf16", "N", "S", "idle", "restarts", "sums", "counts", "x")
    p = [ptr.get(k, FAKE) for k in names]
    return dh.lib().dmi_vq_ema_step(*p, D if ld is None else ld, gamma, R, seed, step, step_dev, M, T, D, None)


def test_ema_step_argument_errors():
    bad = [(dict(M=0), "M must be positive"), (dict(T=0), "positive"), (dict(D=0), "positive"), (dict(ld=56), "ldx"),
           (dict(gamma=0.0), "gamma"), (dict(gamma=1.0), "gamma"), (dict(gamma=-0.1), "gamma"), (dict(gamma=float("nan")), "gamma"),
           (dict(R=-1), "restart_after"), (dict(step=-1), "step"), (dict(codebook_f32=ODD), "aligned"), (dict(codebook_bf16=ODD), "aligned"),
           (dict(S=ODD), "aligned"), (dict(sums=ODD), "aligned"), (dict(x=ODD), "aligned"), (dict(N=ctypes.c_void_p(0x10002)), "aligned"),
           (dict(step_dev=ODD), "aligned")]
    bad += [({k: None}, "null") for k in ("codebook_f32", "codebook_bf16", "N", "S", "idle", "restarts", "sums", "counts", "x")]
    for kw, word in bad:
        assert _ema(**kw) == DMI_ERR_INVALID and _msg().startswith("vq_ema_step") and word in _msg(), (kw, _msg())
    for kw in (dict(D=12, ld=16), dict(D=1024), dict(T=12), dict(T=8192)):
        assert _ema(**kw) == DMI_ERR_UNSUPPORTED and _msg().startswith("vq_ema_step"), (kw, _msg())


# ------------------------------------------------------------------ compile-time resources
def test_new_kernels_use_no_scratch_and_have_no_spills():
    import kres
    mine = {k: v for k, v in kres.usage("vae.hip").items() if "cluster_sums_" in k or "ema_codebook_" in k}
    assert len(mine) == 3, sorted(mine)          # the walk, the combine, the EMA step
    for k, u in mine.items():
        assert u["scratch"] == 0 and u["vspill"] == 0 and u["sspill"] == 0, (k, u)
        assert u["occ"] >= 4, (k, u)             # 512-thread blocks: at least two per CU
