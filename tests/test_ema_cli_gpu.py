"""Weight EMA through the command line on the MI355X: train_dalle.py with "ema_decay" in the config, then generate_dalle.py
--weights ema / raw / auto on its checkpoint, and on the checkpoint of a run without the key.  Every step is a fresh child process
under its own timeout."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(script, args, cwd, timeout):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _ok(r):
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout + r.stderr


def _train(tmp_path, name, **extra):
    """three steps of a one-layer model on the seeded synthetic input; the tokenising VAE keeps its initial weights"""
    vae = json.load(open(os.path.join(ROOT, "configs", "vae_example.json")))
    vae.update(model_path=str(tmp_path / "no_vae_run"))
    json.dump(vae, open(tmp_path / "vae.json", "w"))
    cfg = json.load(open(os.path.join(ROOT, "configs", "dalle_example.json")))
    cfg.update(n_layers=1, n_embd=128, n_heads=2, train_batch_size=4, eval_batch_size=4, predict_batch_size=4, train_steps=3,
               steps_per_checkpoint=3, iterations=1, warmup_steps=1, lr=1e-2, allow_random_vae=True, vae_model=str(tmp_path / "vae.json"),
               model_path=str(tmp_path / name), **extra)
    path = str(tmp_path / (name + ".json"))
    json.dump(cfg, open(path, "w"))
    out = _ok(_child("train_dalle.py", ["--model", path], str(tmp_path), 300))
    assert "model.ckpt-3.pt" in os.listdir(tmp_path / name), os.listdir(tmp_path / name)
    return path, out


def _generate(tmp_path, cfg, out, weights=None):
    args = ["--model", cfg, "--from-eval", "4", "--batch", "4", "--seed", "11", "--no-images", "--out", str(tmp_path / out)]
    return _child("generate_dalle.py", args + (["--weights", weights] if weights else []), str(tmp_path), 300)


def _result(tmp_path, out):
    return np.load(tmp_path / out / "tokens.npy"), json.load(open(tmp_path / out / "generate.json"))


def test_generate_from_a_run_with_an_average(tmp_path):
    cfg, log = _train(tmp_path, "run_ema", ema_decay=0.9)
    assert "ema_decay 0.9" in log, log[-1500:]
    for w in ("ema", "raw", "auto"):
        _ok(_generate(tmp_path, cfg, w, weights=w))
    (t_ema, j_ema), (t_raw, j_raw), (t_auto, j_auto) = (_result(tmp_path, w) for w in ("ema", "raw", "auto"))
    assert j_ema["weights"] == "ema" and j_raw["weights"] == "raw" and j_auto["weights"] == "ema"
    assert t_ema.shape == t_raw.shape == (4, 16) and np.array_equal(t_auto, t_ema)
    assert j_ema["checkpoint"].endswith("model.ckpt-3.pt")


def test_generate_from_a_run_without_an_average(tmp_path):
    cfg, log = _train(tmp_path, "run_plain")
    assert "ema_decay" not in log
    r = _generate(tmp_path, cfg, "e", weights="ema")
    assert r.returncode != 0 and "no weight average" in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    assert not os.path.exists(tmp_path / "e" / "tokens.npy")
    _ok(_generate(tmp_path, cfg, "auto"))                 # no --weights at all: as before the flag existed
    _ok(_generate(tmp_path, cfg, "raw", weights="raw"))
    (t_auto, j_auto), (t_raw, j_raw) = _result(tmp_path, "auto"), _result(tmp_path, "raw")
    assert j_auto["weights"] == "raw" and j_raw["weights"] == "raw" and np.array_equal(t_auto, t_raw)
