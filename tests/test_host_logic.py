"""Host-side mirror of the reference's training scaffolding, on CPU: Estimator loop / checkpoint hooks
(train_dalle.py:71-98, src/model_fns.py:204-229), config loading (src/utils/utils.py:13-17), mesh-shape parsing, schedules
(src/model_fns_tf.py:40-45), summaries (src/utils/utils.py:103-161) -- and the rule that the product path has no CPU
fallback."""
import json
import os

import pytest
import numpy as np
import torch

from src import utils
from src.estimator import (CheckpointSaverHook, Estimator, EstimatorSpec, latest_checkpoint,
                           load_global_step_from_checkpoint_dir)
from src.utils import ModeKeys


def test_fetch_model_params_by_name_and_path(tmp_path):
    p = utils.fetch_model_params("dalle_example")
    assert p["n_embd"] == 512 and p["n_layers"] == 6 and p["text_seq_len"] == 256
    assert p["this_key_does_not_exist"] is None            # reference: defaultdict(lambda: None)
    f = tmp_path / "my.json"
    f.write_text(json.dumps({"model_type": "vae", "lr": 0.5}))
    q = utils.fetch_model_params(str(f))
    assert q["lr"] == 0.5 and q["model_type"] == "vae" and q["missing"] is None
    for name in ("dalle_example", "dalle_coco", "vae_example", "vae_coco"):
        cfg = utils.fetch_model_params(name)
        assert cfg["model_type"] in ("dalle", "vae") and cfg["train_batch_size"] > 0


def test_parse_mesh_shape_and_mode_to_str():
    assert utils.parse_mesh_shape("data:16,model:2") == {"data": 16, "model": 2}
    assert utils.parse_mesh_shape("data:8") == {"data": 8}
    assert utils.parse_mesh_shape("") == {} and utils.parse_mesh_shape(None) == {}
    assert [utils.mode_to_str(m) for m in (ModeKeys.TRAIN, ModeKeys.EVAL, ModeKeys.PREDICT)] == ["train", "eval", "predict"]


def test_param_count_helper(capsys):
    n = utils.get_n_trainable_vars({"a": (3, 4), "b": (5,), "c": ()})
    assert n == 12 + 5 + 1
    assert "N PARAMS" in capsys.readouterr().out


def test_temperature_schedule():
    from src.model_fns_tf import temperature_schedule as ts
    p = {"temp_start": 1.0, "temp": 0.05, "temp_anneal_steps": 100}
    assert ts(0, p) == 1.0 and abs(ts(50, p) - 0.525) < 1e-12 and abs(ts(100, p) - 0.05) < 1e-12 and abs(ts(10 ** 6, p) - 0.05) < 1e-12
    assert ts(7, {"temp": 0.3}) == 0.3 and ts(7, {}) == 1.0


def test_checkpoint_hook_retention_and_latest(tmp_path):
    d = str(tmp_path / "run")
    assert latest_checkpoint(d) is None and load_global_step_from_checkpoint_dir(d) == 0
    state = {"n": 0}
    hook = CheckpointSaverHook(d, save_steps=2, get_state=lambda: {"w": torch.full((3,), float(state["n"]))}, max_to_keep=3)
    for step in range(1, 12):
        state["n"] = step
        hook.after_step(step)
    names = sorted(os.listdir(d), key=lambda s: int(s.split("-")[1].split(".")[0]))
    assert names == ["model.ckpt-6.pt", "model.ckpt-8.pt", "model.ckpt-10.pt"]     # every 2 steps, newest 3 kept
    assert load_global_step_from_checkpoint_dir(d) == 10
    sd = torch.load(latest_checkpoint(d))                                            # weights_only default must work
    assert torch.equal(sd["w"], torch.full((3,), 10.0))
    assert not [f for f in os.listdir(d) if f.endswith(".tmp")]
    CheckpointSaverHook(d, 1, lambda: {"w": torch.zeros(1)}, is_chief=False).after_step(11)   # non-chief ranks never write
    assert load_global_step_from_checkpoint_dir(d) == 10
    CheckpointSaverHook(None, 1, lambda: {}).after_step(5)                           # no model_dir: silently no checkpoints


def test_estimator_loop_contract(tmp_path):
    """train(): model_fn(features, labels, TRAIN, params) per batch, train_op() returns the global step, hooks see every
    step, a final checkpoint is written at max_steps; ONE training input stream lives across train() calls (a train/eval
    loop that calls train() once per checkpoint segment must not replay the stream's head -- ADVICE r01) and is closed by
    close(); evaluate() averages the loss over its own iterator."""
    calls = {"train": 0, "eval": 0, "closed": 0, "host": []}
    state = {"step": 0}
    saver = CheckpointSaverHook(str(tmp_path / "m"), save_steps=1000, get_state=lambda: {"step": torch.tensor(state["step"])})

    class Feed:
        def __init__(self):
            self.i = 0

        def __iter__(self):
            return self

        def __next__(self):
            self.i += 1
            return torch.full((2,), float(self.i)), torch.zeros(2)

        def close(self):
            calls["closed"] += 1

    def model_fn(features, labels, mode, params):
        assert params["marker"] == 42
        if mode == ModeKeys.EVAL:
            calls["eval"] += 1
            return EstimatorSpec(mode=mode, loss=features.mean())

        def train_op():
            calls["train"] += 1
            state["step"] += 1
            return state["step"]
        return EstimatorSpec(mode=mode, loss=features.mean(), train_op=train_op,
                             host_call=(lambda step, **kv: calls["host"].append((step, sorted(kv))), {"loss": features.mean()}),
                             training_hooks=[saver])

    logs = []

    class L:
        info = staticmethod(logs.append)

    est = Estimator(model_fn, str(tmp_path / "m"), {"marker": 42}, log_every=2, logger=L)
    feeds = []

    def input_fn(params):
        feeds.append(Feed())
        return feeds[-1]
    assert est.train(input_fn, max_steps=5) == 5
    assert calls["train"] == 5 and calls["closed"] == 0 and est.params["_input_start_step"] == 0
    assert load_global_step_from_checkpoint_dir(str(tmp_path / "m")) == 5          # final save although 5 % 1000 != 0
    assert [h[0] for h in calls["host"]] == [2, 4] and any("step 4" in m for m in logs)
    assert est.train(input_fn, max_steps=7) == 7                                    # continues from the model's own step
    assert len(feeds) == 1 and feeds[0].i == 7                                      # ... and from the SAME input stream
    out = est.evaluate(lambda params: Feed(), steps=3)
    assert calls["eval"] == 3 and abs(out["loss"] - 2.0) < 1e-6 and calls["closed"] == 1
    est.close()
    assert calls["closed"] == 2


def test_scalar_summaries_to_jsonl(tmp_path):
    utils.scalar_summary("loss", torch.tensor(1.5))
    utils.scalar_summary("lr", 0.25)
    fn, tensors = utils.create_host_call(str(tmp_path))
    fn(7, **tensors)
    rec = json.loads(open(tmp_path / "summaries.jsonl").read().strip().splitlines()[-1])
    assert rec["step"] == 7 and rec["loss"] == 1.5 and rec["lr"] == 0.25


def test_product_path_has_no_cpu_fallback():
    import dalle_hip as dh
    cpu = torch.zeros(8, 8, dtype=torch.bfloat16)
    with pytest.raises(dh.DalleHipError):
        dh.gemm_nt(cpu, 8, cpu, 8, cpu, 8, 8, 8, 64)
    with pytest.raises(dh.DalleHipError):
        dh.layernorm_fwd(cpu, cpu, cpu, cpu, torch.zeros(8), torch.zeros(8), 8, 8)
    if not torch.cuda.is_available():
        from src.dalle_mtf.engine import DalleEngine
        from src.vae_tf import DiscreteVAE
        with pytest.raises(Exception):
            DalleEngine(128, 1, 1, 40, 8, 8, 8, batch_size=1, hparams=dict(lr=1e-3, train_steps=10))
        with pytest.raises(dh.DalleHipError):
            DiscreteVAE(num_tokens=64, dimensions=16, convblocks=[[2, 64]], batch_size=1)


def test_tokenizer_contract_offline():
    from src.data import get_tokenizer
    tok = get_tokenizer(None, vocab_size=50258)
    assert len(tok) == 50258 and tok.encode(tok.pad_token)[0] == 50257     # train_dalle.py:47-49 contract
    with pytest.raises(NotImplementedError):
        get_tokenizer("some_other_tokenizer")


def test_summary_writer_emits_tensorboard_event_file(tmp_path):
    """the event file is TFRecord-framed tensorflow.Event protos: version record first, then scalars (simple_value) and
    PNG-encoded images -- read back here with the repo's own TFRecord reader (CRC-checked) and wire decoder"""
    import glob
    import io
    import struct
    from PIL import Image
    from src.data import tfrecord as tfr
    from src.utils.utils import SummaryWriter
    w = SummaryWriter(str(tmp_path))
    w.scalars(7, loss=1.5, lr=1e-3)
    w.images(7, "input_image", np.random.default_rng(0).random((2, 8, 8, 3), dtype=np.float32))
    (path,) = glob.glob(str(tmp_path / "events.out.tfevents.*"))
    recs = list(tfr.read_records(path, verify_crc=True))
    assert len(recs) == 3
    ev0 = {f: v for f, _, v in tfr._fields(recs[0])}
    assert ev0[3] == b"brain.Event:2"
    ev1 = {f: v for f, _, v in tfr._fields(recs[1])}
    assert ev1[2] == 7 and abs(struct.unpack("<d", ev1[1])[0] - __import__("time").time()) < 60
    vals = {}
    for f, _, value in tfr._fields(ev1[5]):
        fields = {ff: vv for ff, _, vv in tfr._fields(value)}
        vals[fields[1].decode()] = struct.unpack("<f", fields[2])[0]
    assert vals == {"loss": 1.5, "lr": np.float32(1e-3)}
    ev2 = {f: v for f, _, v in tfr._fields(recs[2])}
    tags = []
    for f, _, value in tfr._fields(ev2[5]):
        fields = {ff: vv for ff, _, vv in tfr._fields(value)}
        img = {ff: vv for ff, _, vv in tfr._fields(fields[4])}
        assert (img[1], img[2], img[3]) == (8, 8, 3)
        assert Image.open(io.BytesIO(img[4])).size == (8, 8)
        tags.append(fields[1].decode())
    assert tags == ["input_image/image/0", "input_image/image/1"]


def test_tf_checkpoint_bundle_roundtrip_and_known_constants(tmp_path):
    """TensorFlow V2 checkpoint reader / writer (src/data/tf_checkpoint.py): a multi-block index (many variables), every dtype,
    scalars and empty shapes; CRC failures and a wrong magic are loud; variable selection by scope drops optimizer slots."""
    import struct
    from src.data import tf_checkpoint as tfc
    rng = np.random.default_rng(0)
    V = {f"layer_{i}/attn/q": rng.standard_normal((16, 8)).astype(np.float32) for i in range(120)}
    V.update({"global_step": np.asarray(1234, np.int64), "vae/codebook/codebook": rng.standard_normal((4, 6)).astype(np.float32),
              "vae/codebook/codebook/adam_m": np.zeros((4, 6), np.float32), "half": rng.standard_normal(5).astype(np.float16),
              "ids": np.arange(7, dtype=np.int32), "wide": rng.standard_normal((3, 1, 2)).astype(np.float64)})
    prefix = str(tmp_path / "model.ckpt-1234")
    tfc.save_checkpoint(prefix, V)
    raw = open(prefix + ".index", "rb").read()
    assert struct.unpack("<Q", raw[-8:])[0] == 0xDB4775248B80FB57 and len(raw) > 4096      # more than one data block
    got = tfc.load_checkpoint(prefix)
    assert sorted(got) == sorted(V)
    for k in V:
        assert got[k].dtype == V[k].dtype and got[k].shape == V[k].shape and np.array_equal(got[k], V[k]), k
    assert tfc.list_variables(prefix)["wide"] == ("float64", (3, 1, 2))
    assert tfc.global_step_of(prefix) == 1234
    assert list(tfc.load_model_variables(prefix, scope="vae/")) == ["codebook/codebook"]
    assert "global_step" not in tfc.load_model_variables(prefix)
    open(str(tmp_path / "checkpoint"), "w").write('model_checkpoint_path: "model.ckpt-1234"\n')
    assert tfc.latest_tf_checkpoint(str(tmp_path)) == prefix
    # bfloat16 tensors (the reference's master dtype under bf_16): dtype enum 14, high halves of float32
    bf = (np.asarray([1.0, -2.5, 3.140625], np.float32).view(np.uint32) >> 16).astype("<u2")
    tab = tfc.read_table(prefix + ".index")
    tab[b"bf"] = (tfc._varint(8) + tfc._varint(14) + tfc._ld(2, tfc._shape_proto((3,))) + tfc._varint(32) + tfc._varint(0) +
                  tfc._varint(40) + tfc._varint(6) + tfc._varint(53) + struct.pack("<I", tfc.masked_crc32c(bf.tobytes())))
    open(str(tmp_path / "b.data-00000-of-00001"), "wb").write(bf.tobytes())
    tfc.write_table(str(tmp_path / "b.index"), {b"": tab[b""], b"bf": tab[b"bf"]})
    assert np.array_equal(tfc.load_checkpoint(str(tmp_path / "b"))["bf"], np.asarray([1.0, -2.5, 3.140625], np.float32))
    # corruption is loud
    data = bytearray(open(prefix + ".data-00000-of-00001", "rb").read())
    data[10] ^= 1
    open(prefix + ".data-00000-of-00001", "wb").write(bytes(data))
    with pytest.raises(IOError):
        tfc.load_checkpoint(prefix)
    bad = bytearray(raw)
    bad[100] ^= 1
    open(prefix + ".index", "wb").write(bytes(bad))
    with pytest.raises(IOError):
        tfc.read_table(prefix + ".index")


def test_sampler_uniform_is_strictly_inside_unit_interval():
    """dmi_sample_tokens draws Gumbel noise -log(-log u) from u = (float(h >> 41) + 0.5) * 2^-23 (csrc/elementwise.hip): with 23
    random bits the + 0.5 is exact in fp32, so u stays in [2^-24, 1 - 2^-24] and the noise is finite at both ends.  (With 24
    bits 16777215.5 rounds to 2^24: u == 1, noise +inf, the entry wins regardless of its logit -- round-3 advisor finding.)"""
    f32 = np.float32
    for bits, ok in ((23, True), (24, False)):
        top = f32((1 << bits) - 1)
        u_max = f32(f32(top + f32(0.5)) * f32(1.0 / (1 << bits)))
        u_min = f32(f32(0.5) * f32(1.0 / (1 << bits)))
        assert (u_max < f32(1.0)) == ok and u_min > 0
        if ok:
            noise = -np.log(-np.log(np.array([u_min, u_max], dtype=np.float32)))
            assert np.all(np.isfinite(noise)) and noise[1] < 17.0 and noise[0] > -3.0
    src = open(os.path.join(os.path.dirname(__file__), "..", "dalle-mtf_amd", "csrc", "elementwise.hip")).read()
    assert "(h >> 41) + 0.5f) * (1.0f / 8388608.0f)" in src


def test_dalle_variables_are_the_layouts_reference_variables():
    """DALLE.variables() is built from ParamLayout.reference_variables(): one table of the reference's names and shapes"""
    from src.dalle_mtf.layout import ParamLayout
    from src.dalle_mtf.models import DALLE
    d, L, tv, iv, T, P = 128, 2, 40, 8, 8, 8
    m = DALLE.__new__(DALLE)          # variables() reads the sizes alone: no engine, no device
    m.n_embd, m.n_layers, m.n_heads, m.total_tokens, m.total_seq_dim = d, L, 1, tv + iv + 1, T + P
    from src.dalle_mtf.options import resolve_options
    m.options = resolve_options({}, d, T, P)      # ... and the options record, all off
    lay = ParamLayout(d, L, 1, tv + iv + 1, T + P)
    assert list(m.variables().items()) == [(name, shape) for name, shape, _, _ in lay.reference_variables()]
    v = m.variables()
    assert len(v) == 2 + 13 * L + 4
    assert v["embedding/wte"] == (49, d) and v["positional_embedding/wpe"] == (16, d)
    assert v["to_logits/linear_out/kernel"] == (d, 49) and v["to_logits/linear_out/bias"] == (49,)      # V, not the padded Vp
    assert all(v[f"layer_1/attn/{t}"] == (d, d) for t in "qkvo") and "layer_1/attn/qkv" not in v
    assert v["layer_0/mlp/mlp_linear_1/kernel"] == (d, 4 * d) and v["layer_0/mlp/mlp_linear_2/kernel"] == (4 * d, d)
    # the engine module keeps exporting the layout's names
    from src.dalle_mtf import engine, layout
    assert all(getattr(engine, n) is getattr(layout, n) for n in ("ParamLayout", "adafactor_factored_dims", "adafactor_table", "ALIGN",
                                                                   "_round_up"))
