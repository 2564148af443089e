#!/usr/bin/env python3
"""Landmark bookkeeping + triangulation per frame as a sequence grows: the host time of one frame's step and the
kernel time behind it, after 1, 100 and 1,000 accumulated frames at 3,000 landmarks seen per frame, for 1 and 8 contexts, through
    a  the reference's containers on the host + the stateless velo_triangulate_points (the path before the resident store)
    b  the resident store, one call per context
    c  the resident store with one batch triangulation for all contexts
The walk is tools/landmarks_bench.cpp (C++, through the adaptors' containers), built here with g++.  Host time: a clock around the
step, which ends in a device synchronisation (median of the 5 frames that end at the mark).  Kernel time: a run of its own under
`rocprofv3 --kernel-trace`, from which the launches of the LAST step are summed per kernel (--no-kernels leaves it out).  Needs a GPU.
The claims to test: b does not grow with the frame count while a does; c for 8 contexts beats eight calls of b.
Usage: python tools/landmarks_bench.py [--frames 1 100 1000] [--n 1 8] [--per-frame 3000] [--life 10] [--out profiles/r11_landmarks.txt]"""
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

# launches of one context's step, per mode (c: the gather and the solve are shared by all contexts)
STEP_LAUNCHES = {"a": {"triangulate_wave_kernel": 1}, "b": {"lm_append_kernel": 2, "lm_gather_kernel": 1, "lm_solve_kernel": 1},
                 "c": {"lm_append_kernel": 2, "lm_gather_kernel": 0, "lm_solve_kernel": 0}}
SHARED = {"c": {"lm_gather_kernel": 1, "lm_solve_kernel": 1}}


def compile_driver(out_dir):
    build.build_hip()
    exe = os.path.join(out_dir, "landmarks_bench")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++14", "-O2", "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "tests", "cpp"),
                    os.path.join(ROOT, "tools", "landmarks_bench.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def last_step_kernels(trace_dir, mode, n_ctx):
    """us per kernel name of the last step's launches, from rocprofv3's kernel trace"""
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        return None
    rows = []
    for path in files:
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    out = {}
    for name, per_ctx in STEP_LAUNCHES[mode].items():
        want = per_ctx * n_ctx + SHARED.get(mode, {}).get(name, 0)
        mine = [r for r in rows if name in r["Kernel_Name"]][-want:] if want else []
        out[name] = round(sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in mine) / 1e3, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 100, 1000])
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--modes", nargs="+", default=["a", "b", "c"], choices=["a", "b", "c"])
    ap.add_argument("--per-frame", type=int, default=3000)
    ap.add_argument("--life", type=int, default=10)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"landmark step per frame: {args.per_frame} landmarks seen per frame by 2 cameras, each alive {args.life} frames",
             "host us = one frame's step of ALL contexts (median of the 5 frames ending at the mark); kernel us = the last step's launches"]
    with tempfile.TemporaryDirectory() as td:
        exe = compile_driver(td)
        for n in args.n:
            for mode in args.modes:
                cmd = [exe, mode, str(n), str(args.per_frame), str(args.life)] + [str(f) for f in args.frames]
                out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
                lines += [ln for ln in out.splitlines() if ln.startswith(("step", "done"))]
                print("\n".join(out.splitlines()), flush=True)
                if args.no_kernels or not shutil.which("rocprofv3"):
                    continue
                for fr in args.frames:                     # kernel time: a run of its own per mark, the trace's last step
                    tdir = os.path.join(td, f"trace_{mode}_{n}_{fr}")
                    subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tdir, "--", exe, mode, str(n), str(args.per_frame),
                                    str(args.life), str(fr)], check=True, capture_output=True, text=True, timeout=900)
                    k = last_step_kernels(tdir, mode, n)
                    ln = f"kernels mode={mode} n_ctx={n} frames={fr} " + (" ".join(f"{a}={b}us" for a, b in k.items()) if k else "no trace found")
                    lines.append(ln)
                    print(ln, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
