#!/usr/bin/env python3
"""Producing frameToFrame's visual set for one step: host time of the step for 1 and 8 contexts at 2 cameras x
3,000 keypoints, about 80 % of the ids shared with the previous frame and about half of them added as landmarks, through
    a  the path before the resident frames: velo_landmarks_at_frame read back into a std::map, matchUsingId, the adaptor's gather
       from the nested containers, velo_set_visual
    b  velo_frames_put of the new frame + velo_build_matches, one call per context
    c  velo_frames_put per context + one velo_build_matches_batch
The walk is tools/visual_assembly_bench.cpp (C++, through the adaptors' containers), built here with g++.  Host time: a clock around
the step of ALL contexts, which ends in a device synchronisation; 5 warm-up steps, then the median, minimum and maximum of --reps
steps.  Kernel time: a run of its own under `rocprofv3 --kernel-trace --stats` for modes b and c, from which the fr_* kernels'
average times are read (--no-kernels leaves it out).  Needs a GPU.
The claims to test: b is faster than a at 1 context; c for 8 contexts beats eight calls of b.
Usage: python tools/visual_assembly_bench.py [--n 1 8] [--per-cam 3000] [--reps 200] [--out profiles/r12_visual_assembly.txt]"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import velo_amd  # noqa: E402,F401
from velo_amd import build  # noqa: E402


def compile_driver(out_dir):
    build.build_hip()
    exe = os.path.join(out_dir, "visual_assembly_bench")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++14", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                    os.path.join(ROOT, "tools", "visual_assembly_bench.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def kernel_stats(trace_dir):
    """{kernel: (calls, average us)} of the fr_* launches, from rocprofv3's kernel statistics"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "fr_" in r["Name"]:
                    out[r["Name"].split("(")[0].replace("velo::", "")] = (int(r["Calls"]), round(float(r["AverageNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--modes", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--per-cam", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"visual set of one step: 2 cameras x {args.per_cam} keypoints, ~80 % of the ids shared, ~half of them landmarks",
             f"host us = one step of ALL contexts (5 warm-up steps, then {args.reps}); kernel us = average per launch (rocprofv3 --kernel-trace --stats)"]
    with tempfile.TemporaryDirectory() as td:
        exe = compile_driver(td)
        for n in args.n:
            for mode in args.modes:
                cmd = [exe, mode, str(n), str(args.per_cam), str(args.reps)]
                out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300).stdout
                lines += [ln for ln in out.splitlines() if ln.startswith("step")]
                print(out.strip(), flush=True)
                if args.no_kernels or mode == "a" or not shutil.which("rocprofv3"):
                    continue
                tdir = os.path.join(td, f"trace_{mode}_{n}")
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--"] + cmd, check=True,
                               capture_output=True, text=True, timeout=300)
                k = kernel_stats(tdir)
                ln = f"kernels mode={mode} n_ctx={n} " + (" ".join(f"{a}={c}x{u}us" for a, (c, u) in sorted(k.items())) if k else "no trace found")
                lines.append(ln)
                print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
