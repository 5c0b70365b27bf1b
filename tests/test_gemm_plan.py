"""The GEMM dispatch rules (dalle-mtf_amd/csrc/gemm_plan.h) without a GPU.

1. The host queries of the built library answer as the commit before gemm_plan.h existed: tests/golden/gemm_plan_queries.json
   holds that commit's answers over a grid of shapes and option settings (tests/golden/make_gemm_plan_golden.py wrote it and
   defines the sweep; the CU count falls back to 256 where no device answers, so the answers do not depend on the machine).
2. The plan functions on their own: tests/host/gemm_plan_check.cpp is compiled by the host compiler alone, with the address and
   undefined-behaviour sanitizers, and run as a program of its own -- which kernels the step's products run on, and that no
   weight-gradient plan writes outside the workspace dmi_gemm_tn_workspace_bytes sizes."""
import json
import os
import shutil
import subprocess
import sys

import pytest

import dalle_hip as dh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_gemm_plan_golden as golden  # noqa: E402


@pytest.fixture(scope="module")
def swept():
    """(the sweep on the in-tree library, the committed record); run once, every option back at its value"""
    got = json.loads(json.dumps(golden.sweep(golden.load(dh.LIB_PATH))))
    return got, golden.read()


def test_values_of_the_parent_commit():
    L = golden.load(dh.LIB_PATH)
    assert L.dmi_gemm_tn_workspace_bytes(40960, 512, 50816) == 312823552
    assert L.dmi_gemm_tn_workspace_bytes(40960, 2048, 512) == 67141888
    assert golden.call(L, "dmi_gemm_tn_group_plan", ([2048, 512, 512, 512], [512, 2048, 512, 1536], 40960)) == 5
    assert L.dmi_relu_bits_auto(40960, 2048, 512) == 1 and L.dmi_gemm_nt_ln_auto(40960, 512, 2048) == 1
    assert L.dmi_set_option(b"nt4_lds", 1) == -1 and L.dmi_get_option(b"nope") == -1


def test_sweep_is_the_recorded_one(swept):
    got, want = swept
    assert got["grid_sha256"] == want["grid_sha256"] and got["probe_values"] == want["probe_values"]
    assert [(r["options"], r["query"]) for r in got["rows"]] == [(r["options"], r["query"]) for r in want["rows"]]
    assert len(want["rows"]) == len(golden.SETTINGS) * len(golden.grids()) and len(want["option_rows"]) == len(golden.OPTIONS)


def test_queries_reproduce_the_golden(swept):
    got, want = swept
    grids = golden.grids()
    for g, w in zip(got["rows"], want["rows"]):
        assert len(g["results"]) == len(w["results"]) == len(grids[w["query"]])
        bad = [(a, x, y) for a, x, y in zip(grids[w["query"]], g["results"], w["results"]) if x != y]
        assert not bad, f"{w['query']} under {w['options']}: (arguments, got, recorded) {bad[:5]}"


def test_options_reproduce_the_golden(swept):
    got, want = swept
    for g, w in zip(got["option_rows"], want["option_rows"]):
        assert g == w, w["option"]
    rows = {w["option"]: w for w in want["option_rows"]}
    probes = want["probe_values"]
    assert rows["nope"]["default"] == -1 and all(rc == -1 for rc, _ in rows["nope"]["probes"])                 # unknown name
    assert [rc for rc, _ in rows["nt4_lds"]["probes"]] == [0 if 49152 <= v <= 163840 else -1 for v in probes]  # [49152, 163840]
    assert [rc for rc, _ in rows["reserve_cus"]["probes"]] == [0 if v >= 0 else -1 for v in probes]
    assert [v for _, v in rows["attn_mask_force"]["probes"]] == [1 if v else 0 for v in probes]                # normalised to 0 / 1


def test_plan_functions_stand_alone(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "gemm_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "gemm_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "gemm_plan_check: ok" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
