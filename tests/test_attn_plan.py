"""The attention launch rules (dalle-mtf_amd/csrc/attn_plan.h) without a GPU: tests/host/attn_plan_check.cpp is compiled by the
host compiler alone, with the address and undefined-behaviour sanitizers, and run as a program of its own -- grids, per-XCD
schedule flag and LDS bytes of the persistent kernels, the shape and 32-bit rules, the route of a mask plan and the kernel
choice, each against literals worked out by hand."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_attn_plan_functions_stand_alone(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler found"
    exe = str(tmp_path / "attn_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "host", "attn_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "attn_plan_check: ok" in r.stdout, (r.stdout[-4000:], r.stderr[-4000:])
