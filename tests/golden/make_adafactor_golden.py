"""Generates tests/golden/ref_callsite_adafactor.npz by EXECUTING THE REFERENCE'S OWN get_optimizer with "optimizer": "adafactor"
(src/optimizers.py:19-104, imported from the reference checkout, nothing copied) over the shims of oracle/refshim, for three
consecutive train steps of a small DALL-E (run from the repo root: `python tests/golden/make_adafactor_golden.py`; needs the
reference checkout -- the committed .npz is what travels).

mesh-tensorflow's AdafactorOptimizer is a third-party primitive: the float64 restatement tests/adafactor_ref.py ([MTF-RECALL],
restated from memory of mesh-tensorflow 0.1.18, unchecked against it) is installed as mtfshim.optimize.AdafactorOptimizer at run
time.  What the fixture pins is therefore the reference's side of the call: the argument mapping (weight_decay -> decay_rate,
beta_1, epsilon_1 / epsilon_2 defaults), the global-norm clip applied BEFORE the optimizer, the learning-rate schedule, the slot
variables it creates and carries between steps.

Width 128 with one head (head dim 128) and V = 171 so that the 2-D variables factor: q / k / v / o square (d0 = axis 0), the MLP
kernels and the head kernel with d0 on the long axis, wte [171, 128] with d0 = axis 0; wpe [16, 128] and every 1-D variable use
the full v.  The initial weights are not stored: case_inputs rebuilds them (and the stored tokens) from the seeds through the
oracle's helpers, as for the other ref_callsite fixtures.  Arrays larger than FULL_MAX elements (the 2-D variables and
their momentum slots) are kept as every ROW_STRIDE-th row plus the float64 norm of the whole update (variables) or of the
whole slot, which keeps the file small.  Cases:
  a   weight_decay 0 (no second-moment history), beta_1 0.9, clip 1.0
  b   weight_decay 0.01 (decay rate 0.01), beta_1 0.0 (no momentum slot), clip 0.25"""
import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
from oracle import dalle_oracle as do  # noqa: E402
from oracle.refshim import available, harness, mtfshim, tfshim  # noqa: E402
import adafactor_ref as ar  # noqa: E402

OUT = os.path.join(HERE, "ref_callsite_adafactor.npz")
FULL_MAX = 4096   # arrays up to this many elements are stored whole; larger ones as every ROW_STRIDE-th row + a float64 norm
ROW_STRIDE = 16
STEPS = 3
BASE = dict(n_embd=128, text_vocab_size=150, image_vocab_size=20, text_seq_len=8, image_seq_len=8, n_layers=1, n_heads=1,
            bf_16=False, lr=2e-2, train_steps=1000, warmup_steps=4, gradient_clipping=1.0, optimizer="adafactor")
CASES = {
    "a": dict(hp=dict(BASE, weight_decay=0.0, beta_1=0.9), batch=2, step=10, seeds=(21, 5, 6)),
    "b": dict(hp=dict(BASE, weight_decay=0.01, beta_1=0.0, gradient_clipping=0.25, lr_decay="linear"), batch=2, step=2,
              seeds=(22, 7, 8)),
}


class AdafactorOptimizer(mtfshim.Optimizer):
    """mtf.optimize.AdafactorOptimizer's constructor as get_optimizer calls it; apply_grad = tests/adafactor_ref.apply_grad on the
    slot variables <var>_slot_vr / _slot_vc / _slot_v / _slot_m (zero-initialised, carried between steps by the generator)"""

    def __init__(self, learning_rate, decay_rate=0.0, beta1=0.0, epsilon1=1e-30, epsilon2=1e-3):
        self.learning_rate, self.decay_rate, self.beta1 = learning_rate, decay_rate, beta1
        self.epsilon1, self.epsilon2 = epsilon1, epsilon2

    def apply_grad(self, grad, var):
        if grad is None:
            return []
        shape = var.shape.to_integer_list
        slots = OrderedDict()
        slot_vars = OrderedDict()
        fd = ar.factored_dims(shape)
        for sname in ar.slot_names(var.name, shape, self.beta1):
            kind = sname.rsplit("_", 1)[1]
            dims = {"vr": [var.shape.dims[fd[1]]] if fd else None, "vc": [var.shape.dims[fd[0]]] if fd else None}.get(kind, var.shape.dims)
            t = mtfshim.get_variable(var.mesh, sname, mtfshim.Shape(dims), initializer=tfshim.zeros_initializer(), trainable=False)
            slot_vars[sname] = t.operation
            slots[sname] = t.operation.master.detach().double().numpy().copy()
        lr = float(self.learning_rate.value.detach().double())
        w = var.master.detach().double().numpy()
        g = grad.value.detach().double().numpy()
        new_w = ar.apply_grad(var.name, w, g, slots, lr, self.decay_rate, self.beta1, self.epsilon1, self.epsilon2)
        ops = [mtfshim._Assign(var, torch.tensor(new_w, dtype=torch.float32))]
        for sname, op in slot_vars.items():
            ops.append(mtfshim._Assign(op, torch.tensor(slots[sname], dtype=torch.float32)))
        return ops


def case_inputs(case):
    hp = case["hp"]
    cfg = do.DalleConfig(hp["n_embd"], hp["text_vocab_size"], hp["image_vocab_size"], hp["text_seq_len"], hp["image_seq_len"],
                         hp["n_layers"], hp["n_heads"])
    ws, ts, is_ = case["seeds"]
    weights = do.init_params(cfg, seed=ws, perturb=0.05)
    text = do.synthetic_captions(case["batch"], cfg.text_seq_len, cfg.text_vocab_size, seed=ts)
    img = do.synthetic_image_tokens(case["batch"], cfg.image_seq_len, cfg.image_vocab_size, seed=is_)
    return cfg, weights, do.assemble_tokens(text, img, cfg.text_vocab_size)


def sample(a):
    """the part of an array the fixture keeps: all of it up to FULL_MAX elements, otherwise every ROW_STRIDE-th row (axis 0)"""
    a = np.asarray(a)
    return a if a.size <= FULL_MAX else a[::ROW_STRIDE]


def store(out, name, value, w0=None):
    """after:<name> = sample(value); for a sampled array also norm:<name> = ||value - w0|| (the update of a variable) or ||value||
    (a slot), over the whole array in float64"""
    value = np.asarray(value, np.float32)
    out["after:" + name] = sample(value)
    if value.size > FULL_MAX:
        ref = value.astype(np.float64) - (0.0 if w0 is None else np.asarray(w0, np.float64))
        out["norm:" + name] = np.float64(np.linalg.norm(ref))


def fixture_case(blob, name):
    """(after, norms) of a case: name -> stored sample, name -> whole-array norm (sampled arrays only)"""
    pre = name + "/after:"
    after = {k[len(pre):]: v for k, v in blob.items() if k.startswith(pre)}
    pre = name + "/norm:"
    return after, {k[len(pre):]: float(v) for k, v in blob.items() if k.startswith(pre)}


def run_case(case):
    cfg, weights, tokens = case_inputs(case)
    state = OrderedDict((k, np.asarray(v, np.float32)) for k, v in weights.items())
    losses, lrs = [], []
    for i in range(STEPS):
        r = harness.run_dalle_step(case["hp"], state, tokens, global_step=case["step"] + i, return_logits=False)
        losses.append(float(r["loss"]))
        lrs.append(float(r["lr"]))
        state = OrderedDict(state)
        state.update(r["updated"])
    out = {"tokens": tokens, "loss": np.array(losses, np.float32), "lr": np.array(lrs, np.float32)}
    for k, v in state.items():
        store(out, k, v, weights.get(k))
    return out


def main():
    assert available(), "needs the reference checkout"
    saved = getattr(mtfshim.optimize, "AdafactorOptimizer", None)
    mtfshim.optimize.AdafactorOptimizer = AdafactorOptimizer
    try:
        blob = {"cases": np.array(json.dumps(CASES))}
        for name, case in CASES.items():
            for k, v in run_case(case).items():
                blob[name + "/" + k] = v
    finally:
        if saved is None:
            del mtfshim.optimize.AdafactorOptimizer
        else:
            mtfshim.optimize.AdafactorOptimizer = saved
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, sum(v.nbytes for v in blob.values()), "bytes")


if __name__ == "__main__":
    main()
