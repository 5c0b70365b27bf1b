#!/usr/bin/env python
"""Writes tests/golden/vae_lowering.json: what DiscreteVAE derives on the host from its layer list, read off constructed models
on a GPU machine -- the flat parameter layout, the derived weight copies and their offsets, the tables of the two batched refresh
launches, and the scratch sizes -- for five configurations (tests/test_vae_lowering.py names what each one reaches).  Only
attributes of the model are read, so the file can be regenerated from any revision that keeps them:

    python tests/golden/make_vae_lowering_golden.py [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def configurations():
    shipped = {}
    for name in ("vae_example", "vae_coco"):
        p = json.load(open(os.path.join(ROOT, "configs", name + ".json")))
        shipped[name] = dict(num_tokens=p["num_tokens"], dimensions=p["dataset"]["image_size"], convblocks=p["convblocks"], batch_size=1)
    return dict(shipped,
                unaligned=dict(num_tokens=64, dimensions=16, convblocks=[[2, 16], [2, 64]], batch_size=2),
                nonpow2=dict(num_tokens=64, dimensions=24, convblocks=[[2, 64], [2, 128]], batch_size=2),
                stacked=dict(num_tokens=64, dimensions=32, convblocks=[[2, 64], [2, 64]], batch_size=2, stack_factor=2))


def describe(vae):
    views = dict(wf=vae.wf, wd=vae.wd, cb={"codebook_t": vae.codebook_t})
    copies = []
    for (kind, name, q), off in vae._wc_off.items():        # insertion order = layout order
        v = vae.wp[name][q] if kind == "wp" else views[kind][name]
        copies.append([kind, name, q, off, v.shape[0], v.shape[1]])
    T = vae._refresh_tables
    return dict(offset=vae.offset, shape={k: list(v) for k, v in vae.shape.items()}, total=vae.total,
                weight_copies=copies, wcopies_numel=vae.wcopies.numel(),
                tr=T["tr"].cpu().tolist(), tiles=T["tiles"], ga=T["ga"].cpu().tolist() if T["ga"] is not None else None,
                blocks=T["blocks"], padded=[list(p) for p in T["padded"]],
                col_numel=vae.col.numel(), ws_bytes=vae.ws.numel(), ws_cs_bytes=vae.ws_cs.numel(),
                ws_pool_slot_bytes=vae.ws_pool[0].numel(), ws_pool_slots=len(vae.ws_pool))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "vae_lowering.json"))
    a = ap.parse_args()
    sys.path[:0] = [os.path.join(ROOT, "dalle-mtf_amd"), ROOT]
    from src.vae_tf import DiscreteVAE
    out = {}
    for name, cfg in configurations().items():
        vae = DiscreteVAE(**cfg)
        vae.init_params(seed=1)       # (the refresh tables are built by the first refresh_compute_copies)
        out[name] = dict(config=cfg, **describe(vae))
        del vae
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}:{json.dumps(v, sort_keys=True, separators=(',', ':'))}" for k, v in out.items()) + "\n}\n")
    print("wrote", a.out, os.path.getsize(a.out), "bytes")


if __name__ == "__main__":
    main()
