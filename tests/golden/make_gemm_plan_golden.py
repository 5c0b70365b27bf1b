#!/usr/bin/env python
"""Sweeps the host-side GEMM queries of libdalle_hip (no device needed: the CU count falls back to 256) and writes
tests/golden/gemm_plan_queries.json.  tests/test_gemm_plan.py runs the same sweep on the in-tree library and compares.

The committed file was written from the library of the commit before csrc/gemm_plan.h existed, so it pins that commit's
dispatch rules.  Regenerate it only when a rule is meant to change:

    DALLE_HIP_LIB=/path/to/libdalle_hip.so python tests/golden/make_gemm_plan_golden.py

One row per (option setting, query): the results in the order of the argument grid that `grids()` returns; the file pins the
grid by its SHA-256, and a row under a changed option that equals the row under the defaults is written as "default" (`pack` /
`read`).  Option rows: for each name the default, then (set status, value read back) per probe value."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gemm_plan_queries.json")

MS = [64, 2560, 40960, 163840]
WIDTHS = [128, 256, 384, 512, 768, 1024, 1536, 2048]
VOCAB = [50816, 58368]           # the headline head and the larger vocabulary's, both padded to 64 columns
OPTIONS = ["nt4", "nt8", "tn_tail", "tn_wide", "nt4_lds", "nt8p", "ntr", "cstream", "cstream_min_mb", "cstream_nt_min_mb", "nt8p_max_k",
           "relu_bits", "res16", "skinny", "nt8_min_k", "tn8", "tn8_max_tiles", "attn_xcd", "attn_mask_force", "attn_fwd", "attn_bwd",
           "reserve_cus", "nope"]
PROBES = [-1, 0, 1, 2, 3, 7, 49151, 49152, 65536, 163840, 163841]
# the options that feed the queries, one changed at a time from the defaults
SETTINGS = [{}] + [{k: v} for k, vs in (("tn8", (1, 2)), ("tn_wide", (0,)), ("nt8p", (0, 2, 3)), ("relu_bits", (0,)),
                                        ("nt8p_max_k", (512, 2048)), ("reserve_cus", (16,))) for v in vs]


def grids():
    pairs = [(a, b) for a in WIDTHS for b in WIDTHS] + [(w, v) for v in VOCAB for w in (512, 2048)] + [(v, w) for v in VOCAB for w in (512, 2048)]
    four = lambda d: ([4 * d, d, d, d], [d, 4 * d, d, 3 * d])   # noqa: E731  (a block's FFN-1, FFN-2, out-projection, QKV gradients)
    groups = []
    for d in (128, 256, 512, 1024, 2048):
        I, J = four(d)
        groups += [(I, J), (I[:2], J[:2]), (I[2:], J[2:]), (I[:1], J[:1])]
    groups += [([], []), ([512] * 5, [512] * 5)]                # outside 1..4 problems: 0
    return {
        "dmi_gemm_tn_workspace_bytes": [(m, i, j) for m in MS for i, j in pairs],
        "dmi_gemm_tn_group_plan": [(i, j, m) for m in MS + [0] for i, j in groups],
        "dmi_relu_bits_auto": [(m, n, k) for m in MS for n, k in pairs],
        "dmi_gemm_nt_ln_auto": [(m, n, k) for m in MS + [0, 4194304] for n, k in pairs],
        "dmi_relu_bits_bytes": [(m, n) for m in MS for n in WIDTHS + VOCAB + [8, 72]],
        "dmi_gemm_nt_lnbwd_parts": [(m,) for m in MS + [1, 159, 160, 161]],
        "dmi_gemm_nt_splitk_workspace_bytes": [(m, n, s) for m in MS for n in WIDTHS for s in (1, 2, 4, 16)],
    }


def load(path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "dalle-mtf_amd"))
    from dalle_hip import abi
    L = ctypes.CDLL(path)
    abi.declare(L)          # the signatures of include/dalle_hip.h
    return L


def call(L, name, args):
    if name == "dmi_gemm_tn_group_plan":
        I, J, M = args
        arr = lambda v: (ctypes.c_int * max(len(v), 1))(*v)   # noqa: E731
        return int(L.dmi_gemm_tn_group_plan(arr(I), arr(J), len(I), M))
    return int(getattr(L, name)(*args))


def sweep(L):
    """the whole record as a JSON-able dict; leaves every option at the value it had"""
    g = grids()
    rows = []
    for setting in SETTINGS:
        saved = {k: L.dmi_get_option(k.encode()) for k in setting}
        for k, v in setting.items():
            assert L.dmi_set_option(k.encode(), v) == 0, (k, v)
        try:
            rows += [dict(options=setting, query=name, results=[call(L, name, a) for a in args]) for name, args in g.items()]
        finally:
            for k, v in saved.items():
                L.dmi_set_option(k.encode(), v)
    opts = []
    for name in OPTIONS:
        default = L.dmi_get_option(name.encode())
        tried = []
        for v in PROBES:
            rc = L.dmi_set_option(name.encode(), v)
            tried.append([rc, L.dmi_get_option(name.encode())])
        if default >= 0:
            L.dmi_set_option(name.encode(), default)
        opts.append(dict(option=name, default=default, probes=tried))
    grid_sha = hashlib.sha256(json.dumps(g, sort_keys=True).encode()).hexdigest()
    return dict(grid_sha256=grid_sha, probe_values=PROBES, rows=rows, option_rows=opts)


def pack(rec):
    base = {r["query"]: r["results"] for r in rec["rows"] if not r["options"]}
    same = lambda r: r["options"] and r["results"] == base[r["query"]]   # noqa: E731
    return dict(rec, rows=[dict(r, results="default") if same(r) else r for r in rec["rows"]])


def read(path=OUT):
    """the committed record with every "default" row written out again"""
    rec = json.load(open(path))
    base = {r["query"]: r["results"] for r in rec["rows"] if not r["options"]}
    return dict(rec, rows=[dict(r, results=base[r["query"]]) if r["results"] == "default" else r for r in rec["rows"]])


def main():
    path = os.environ.get("DALLE_HIP_LIB")
    if not path:
        sys.exit("set DALLE_HIP_LIB to the library to record")
    with open(OUT, "w") as f:
        json.dump(pack(sweep(load(path))), f, separators=(",", ":"))
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
