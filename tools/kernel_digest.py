#!/usr/bin/env python3
"""Dev tool (no GPU needed): one digest line per kernel of a build, to show that a change of the kernel sources left the machine code alone.

    python tools/kernel_digest.py list [--csrc DIR] [--diag] > listing     # DIR: another tree's csrc (default: this tree's)
    python tools/kernel_digest.py diff OLD NEW                              # added / removed / changed kernels; exit status 1 on a change

`list` compiles every unit of build.KERNEL_UNITS with the flags only it gets (and -DVELO_DIAGNOSTICS with --diag) to gfx950 assembly
(--cuda-device-only -S) and prints, per kernel: unit, demangled name, a digest of its instruction text (comments stripped, local label
numbers renumbered in order of appearance -- they count the functions before it in the unit) and a digest of its .amdhsa_kernel ...
.end_amdhsa_kernel block (registers, LDS, scratch, kernel-argument size).  Nothing else of the assembly is looked at.
`diff` counts per unit; kernels are keyed by name alone, so one that moved to another unit still compares."""
import argparse, collections, hashlib, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import velo_amd
from velo_amd import build

_LOCAL = re.compile(r"\.L[A-Za-z_]+[0-9][0-9_]*")


def _digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16]


def _code_digest(lines):
    seen = {}
    out = []
    for line in lines:
        line = line.split(";", 1)[0].strip()
        if line:
            out.append(_LOCAL.sub(lambda m: seen.setdefault(m.group(0), f".L{len(seen)}"), " ".join(line.split())))
    return _digest(out)


def kernels_of(asm):
    """{mangled name: (code digest, descriptor digest)} of one unit's assembly text"""
    lines = asm.splitlines()
    label = {l.split(":", 1)[0]: i for i, l in enumerate(lines) if l[:1] not in ("", "\t", " ", ";", ".") and ":" in l}
    found = {}
    for i, l in enumerate(lines):
        if not l.strip().startswith(".amdhsa_kernel "):
            continue
        name = l.split()[1]
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        first = label[name] + 1
        last = next(j for j in range(first, i) if lines[j].lstrip().startswith(".section"))      # the descriptor's section ends the code
        found[name] = (_code_digest(lines[first:last]), _digest([" ".join(x.split()) for x in lines[i:end + 1]]))
    return found


def listing(csrc, diag):
    flags = [f for f in build.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + (["-DVELO_DIAGNOSTICS"] if diag else [])
    inc = os.path.join(os.path.dirname(os.path.dirname(csrc)), "include")          # csrc includes "../../include/velo_hip.h" by itself; -I as build.py has it
    with tempfile.TemporaryDirectory() as tmp:
        def one(unit):
            s = os.path.join(tmp, unit + ".s")
            subprocess.run(["hipcc", *flags, *build.SOURCES[unit], "-I", inc, "--cuda-device-only", "-S", "-o", s, os.path.join(csrc, unit)],
                           check=True, stderr=subprocess.DEVNULL)
            with open(s) as f:
                return kernels_of(f.read())
        with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
            per_unit = list(pool.map(one, build.KERNEL_UNITS))
    names = [n for k in per_unit for n in k]
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    plain = dict(zip(names, plain))
    for unit, k in zip(build.KERNEL_UNITS, per_unit):
        for name, (code, desc) in k.items():
            print(f"{unit}\t{plain[name]}\t{code}\t{desc}")


def read(path):
    with open(path) as f:
        rows = [l.rstrip("\n").split("\t") for l in f if l.strip()]
    return {name: (unit, code, desc) for unit, name, code, desc in rows}


def diff(old_path, new_path):
    old, new = read(old_path), read(new_path)
    count = collections.defaultdict(lambda: collections.Counter())
    for name in sorted(old.keys() | new.keys()):
        unit = (old.get(name) or new[name])[0]
        if name not in new:
            kind = "removed"
        elif name not in old:
            kind = "added"
        else:
            count[unit]["compared"] += 1
            kind = "equal" if old[name][1:] == new[name][1:] else "changed"
            if kind == "changed":
                what = [w for w, a, b in zip(("code", "descriptor"), old[name][1:], new[name][1:]) if a != b]
                print(f"changed ({' + '.join(what)})  {unit}  {name}")
        count[unit][kind] += 1
        if kind in ("removed", "added"):
            print(f"{kind}  {unit}  {name}")
    total = collections.Counter()
    for unit in sorted(count):
        c = count[unit]
        total.update(c)
        print(f"{unit:26s} compared {c['compared']:3d}  equal {c['equal']:3d}  changed {c['changed']:3d}  removed {c['removed']:3d}  added {c['added']:3d}")
    print(f"{'total':26s} compared {total['compared']:3d}  equal {total['equal']:3d}  changed {total['changed']:3d}  removed {total['removed']:3d}  added {total['added']:3d}")
    return 1 if total["changed"] or total["added"] or total["removed"] else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("list")
    p.add_argument("--csrc", default=build.CSRC)
    p.add_argument("--diag", action="store_true")
    p = sub.add_parser("diff")
    p.add_argument("old")
    p.add_argument("new")
    a = ap.parse_args()
    sys.exit(listing(os.path.abspath(a.csrc), a.diag) if a.cmd == "list" else diff(a.old, a.new))
