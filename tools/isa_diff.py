#!/usr/bin/env python3
"""Compare the kernels of two gfx950 assembly files, one line per kernel: registers, scratch, LDS and instruction text.

  hipcc <dalle_hip/build.py FLAGS> --cuda-device-only -S csrc/attention.hip -o new.s      (the same for the other revision: old.s)
  tools/isa_diff.py old.s new.s ['old name=new name' ...]  [--show SUBSTRING]

Kernels are matched by demangled name (c++filt) without the argument list; a rename is given as 'old=new'.  A kernel's text runs
from its label to its s_endpgm; comments, the symbol itself and the function index of local labels (.LBB<n>_<m>) are naming only
and are dropped.  Exit status 1 if any kernel differs or is missing."""
import difflib, re, shutil, subprocess, sys

FIELDS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    text = open(path).read()
    lines = text.split("\n")
    out = {}
    for blk in text[text.index("amdhsa.kernels:"):].split("\n  - .")[1:]:
        sym = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta = " / ".join(re.search(r"\." + f + r":\s+(\d+)", blk).group(1) for f in FIELDS)
        body = []
        for ln in lines[next(i for i, l in enumerate(lines) if l.startswith(sym + ":")) + 1:]:
            ln = re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip().replace(sym, "SYM"))
            if ln:
                body.append(ln)
            if ln == "s_endpgm":
                break
        out[sym] = (meta, body)
    filt = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    names = subprocess.run([filt], input="\n".join(out), capture_output=True, text=True).stdout.split("\n") if filt else list(out)
    return {re.sub(r"^void |\(.*$", "", n): v for n, v in zip(names, out.values())}


def main():
    args = [a for a in sys.argv[1:] if a != "--show"]
    show = sys.argv[sys.argv.index("--show") + 1] if "--show" in sys.argv else None
    if show:
        args.remove(show)
    old, new = kernels(args[0]), kernels(args[1])
    rename = dict(a.split("=") for a in args[2:])
    bad = 0
    print("kernel: VGPR / SGPR / scratch B / static LDS B, old -> new; instruction text")
    for name in sorted(old):
        (m0, b0), (m1, b1) = old[name], new.get(rename.get(name, name), ("missing", []))
        ops = [o for o in difflib.SequenceMatcher(None, b0, b1, autojunk=False).get_opcodes() if o[0] != "equal"]
        n = sum(max(i2 - i1, j2 - j1) for _, i1, i2, j1, j2 in ops)
        bad += bool(n) or m0 != m1
        print(f"{name} -> {rename.get(name, name)}: {m0} -> {m1}; " + (f"{n} of {len(b0)} instructions differ" if n else f"identical ({len(b0)} instructions)"))
        if n and show and show in name:
            print("\n".join("    " + l for l in difflib.unified_diff(b0, b1, lineterm="", n=2)))
    sys.exit(1 if bad else 0)


main()
