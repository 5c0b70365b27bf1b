"""Generates tests/golden/ref_callsite_gelu.npz by EXECUTING THE REFERENCE'S OWN DALLE with activation_fn = gelu (src/dalle_mtf/models.py,
imported from the reference checkout over the shims of oracle/refshim, nothing copied) for one forward / backward of a small model
(run from the repo root: `python tests/golden/make_gelu_golden.py`; needs the reference checkout -- the committed .npz is what travels).

oracle/refshim/harness.run_dalle_step builds DALLE the way src/model_fns.py does, which never passes activation_fn; this script makes
the same calls itself with activation_fn given.  mtf.gelu is a third-party primitive: it is restated here in float64 (the tanh form,
[MTF-RECALL] from memory of mesh-tensorflow 0.1.18, unchecked against it) as a mtfshim._unary.  What the fixture pins is the
reference's side of the call: where activation_fn applies (the MLP's hidden layer only, models.py:317-324), and the loss and
gradients that follow from it.  The initial weights are not stored: the test rebuilds them from the seeds through the oracle's
helpers, as for the other ref_callsite fixtures."""
import json
import math
import os
import sys
from collections import OrderedDict, defaultdict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle import dalle_oracle as do  # noqa: E402
from oracle.refshim import available, installed, mtfshim, reference_module, tfshim  # noqa: E402

OUT = os.path.join(HERE, "ref_callsite_gelu.npz")
CASE = dict(n_embd=64, text_vocab_size=150, image_vocab_size=20, text_seq_len=8, image_seq_len=8, n_layers=1, n_heads=1,
            batch=2, seed=31, perturb=0.05, text_seed=5, image_seed=6)


def _gelu64(v):
    x = v.double()
    return (0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))).to(v.dtype)


def gelu(x, name=None):
    """mtf.gelu over the shim: float64 tanh form, autograd through torch"""
    return mtfshim._unary(_gelu64, x, name=name or "gelu")


def run(case):
    cfg = do.DalleConfig(case["n_embd"], case["text_vocab_size"], case["image_vocab_size"], case["text_seq_len"],
                         case["image_seq_len"], case["n_layers"], case["n_heads"])
    weights = do.init_params(cfg, seed=case["seed"], perturb=case["perturb"])
    text = do.synthetic_captions(case["batch"], cfg.text_seq_len, cfg.text_vocab_size, seed=case["text_seed"])
    img = do.synthetic_image_tokens(case["batch"], cfg.image_seq_len, cfg.image_vocab_size, seed=case["image_seed"])
    tokens = do.assemble_tokens(text, img, cfg.text_vocab_size)
    with installed():
        models = reference_module("dalle_mtf.models")
        params = defaultdict(lambda: None, dict(case, bf_16=False, num_microbatches=1))
        mtfshim.inject_variables({k: np.asarray(v) for k, v in weights.items()})
        tfshim.set_global_step(0)
        model = models.DALLE(n_embd=cfg.n_embd, text_vocab_size=cfg.text_vocab_size, image_vocab_size=cfg.image_vocab_size,
                             text_seq_len=cfg.text_seq_len, image_seq_len=cfg.image_seq_len, n_layers=cfg.n_layers,
                             n_heads=cfg.n_heads, batch_size=case["batch"], bf_16=False, mode="train", params=params,
                             activation_fn=gelu)
        graph = mtfshim.Graph()
        mesh = mtfshim.Mesh(graph, "my_mesh")
        shape = mtfshim.Shape([model.dimensions["batch_dim"], model.dimensions["total_seq_dim"]])
        features = {"tokens": mtfshim.import_fully_replicated(mesh, torch.as_tensor(tokens.astype(np.int32)), shape, name="text_inputs")}
        loss, _ = model.forward(features, return_loss=True)
        variables = graph.trainable_variables
        raw = mtfshim.gradients([loss], [v.outputs[0] for v in variables])
        out = OrderedDict(case=np.array(json.dumps(case)), tokens=tokens, loss=loss.value.detach().numpy().astype(np.float32))
        for v, g in zip(variables, raw):
            out["grad:" + v.name] = g.value.detach().numpy().astype(np.float32)
    return out


def main():
    assert available(), "needs the reference checkout"
    blob = run(CASE)
    np.savez_compressed(OUT, **blob)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; loss", float(blob["loss"]))


if __name__ == "__main__":
    main()
