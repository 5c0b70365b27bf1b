"""Per-kernel / per-grid breakdown of the last N steps of a rocprofv3 kernel_trace.csv of bench.py (steps are delimited
by the adam_kernel launch): python tools/trace_summary.py <kernel_trace.csv> [nsteps]

python tools/trace_summary.py --signatures <kernel_trace.csv> [--digest]: one line per dispatch, in dispatch order: kernel name |
grid | block | LDS bytes -- what a launcher decides; two builds whose host code makes the same choices print the same text.
--digest: the distinct lines with their counts, the number of dispatches and SHA-256 of the full text (small enough to keep)."""
import collections, csv, hashlib, sys
rows = list(csv.DictReader(open([a for a in sys.argv[1:] if not a.startswith("--")][0])))
if "--signatures" in sys.argv:
    sig = [" | ".join((r["Kernel_Name"], "x".join(r["Grid_Size_" + d] for d in "XYZ"), "x".join(r["Workgroup_Size_" + d] for d in "XYZ"),
                       r["LDS_Block_Size"])) for r in sorted(rows, key=lambda r: int(r["Dispatch_Id"]))]
    if "--digest" in sys.argv:
        print(f"{len(sig)} dispatches, sha256 of the per-dispatch text {hashlib.sha256(''.join(s + chr(10) for s in sig).encode()).hexdigest()}")
        sig = [f"{n:7d}  {s}" for s, n in sorted(collections.Counter(sig).items())]
    print("\n".join(sig))
    sys.exit(0)
nsteps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
idx = [i for i, r in enumerate(rows) if r["Kernel_Name"].startswith("adam_kernel")]
lo, hi = idx[-nsteps - 1] + 1, idx[-1] + 1
acc = collections.OrderedDict()
for r in rows[lo:hi]:
    key = (r["Kernel_Name"][:46], r["Grid_Size_X"], r["Grid_Size_Y"])
    a = acc.setdefault(key, [0, 0])
    a[0] += 1
    a[1] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
tot = sum(v[1] for v in acc.values()) / nsteps
span = (int(rows[hi - 1]["End_Timestamp"]) - int(rows[lo]["Start_Timestamp"])) / nsteps
print(f"kernel time / step {tot/1e6:.3f} ms, wall span / step {span/1e6:.3f} ms (profiled run)")
for k, v in sorted(acc.items(), key=lambda kv: -kv[1][1]):
    if v[1] / nsteps < 4000:
        continue
    print(f"{k[0]:46s} grid=({k[1]},{k[2]}) n/step={v[0]/nsteps:5.1f} avg={v[1]/v[0]/1e3:8.1f} us  per-step={v[1]/nsteps/1e3:8.1f} us")
