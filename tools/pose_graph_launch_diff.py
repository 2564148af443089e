"""Dev tool (no GPU needed): compares two rocprofv3 output directories of tools/pose_graph_launch_seq.py -- the kernels in start order by name,
grid, workgroup, LDS and scratch size; the copies in start order by direction (CSV) and by operation, kind and bytes (JSON)."""
import csv
import glob
import json
import os
import sys


def rows(d, suffix):
    files = sorted(glob.glob(os.path.join(d, "**", "*" + suffix), recursive=True))
    out = []
    for f in files:
        with open(f, newline="") as fh:
            out += list(csv.DictReader(fh))
    out.sort(key=lambda r: int(r["Start_Timestamp"]))
    return files, out


def keyed(rs, want):
    cols = [c for c in want if rs and c in rs[0]]
    return cols, [tuple(r[c] for c in cols) for r in rs]


KERNEL = ["Kernel_Name", "Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z", "Workgroup_Size_X", "Workgroup_Size_Y", "Workgroup_Size_Z", "LDS_Block_Size", "Scratch_Size"]
COPY = ["Direction", "Bytes", "Size", "Copy_Size", "Size_Bytes"]
ok = True
for suffix, want, what in (("kernel_trace.csv", KERNEL, "kernels"), ("memory_copy_trace.csv", COPY, "copies")):
    fa, a = rows(sys.argv[1], suffix)
    fb, b = rows(sys.argv[2], suffix)
    ca, ka = keyed(a, want)
    cb, kb = keyed(b, want)
    same = ka == kb and ca == cb
    ok = ok and same and len(ka) > 0
    print(f"{what}: first {len(ka)}, second {len(kb)}; compared in start order on {ca}: {'IDENTICAL' if same else 'DIFFERENT'}")
    if a:
        print(f"   all columns of the trace: {list(a[0].keys())}")
    if not same:
        for i, (x, y) in enumerate(zip(ka, kb)):
            if x != y:
                print(f"   first difference at {i}: first {x} / second {y}")
                break
    names = {}
    for k in ka:
        names[k[0]] = names.get(k[0], 0) + 1
    for nme, cnt in sorted(names.items(), key=lambda t: -t[1])[:40]:
        print(f"   {cnt:6d}  {nme[:150]}")
def copies_json(d):
    out = []
    for f in sorted(glob.glob(os.path.join(d, "**", "*results.json"), recursive=True)):
        with open(f) as fh:
            doc = json.load(fh)
        for tool in doc.get("rocprofiler-sdk-tool", []):
            out += tool.get("buffer_records", {}).get("memory_copy", [])
    out.sort(key=lambda r: r.get("start_timestamp", 0))
    return out


ja, jb = copies_json(sys.argv[1]), copies_json(sys.argv[2])
if ja or jb:
    keys = [k for k in ("operation", "kind", "bytes") if ja and k in ja[0]]
    ka, kb = [tuple(r.get(k) for k in keys) for r in ja], [tuple(r.get(k) for k in keys) for r in jb]
    print(f"copies (json): first {len(ka)}, second {len(kb)}; compared on {keys}: {'IDENTICAL' if ka == kb else 'DIFFERENT'}; the records' keys {sorted(ja[0].keys()) if ja else []}")
    print(f"   first's: {ka[:12]}")
    ok = ok and ka == kb
else:
    print("copies (json): no json record found")
print("verdict:", "the launch sequences are identical" if ok else "NOT identical (or empty)")
