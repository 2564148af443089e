#!/usr/bin/env python3
"""The prune of the current frame to a registration's good matches: host time per prune at 2 cameras x 3,000
keypoints with descriptor rows, about half of them kept (frame2 holds every second keypoint of frame1, with the same depth points, so
every record passes the gate at the identity pose), through
    a  the path before the resident prune: velo_get_good_matches, the containers cut on the host (vectorised numpy, cheaper than the
       reference's loop, so (a) is flattered), velo_frames_put + velo_frames_put_descriptors of every camera, a synchronisation
    b  velo_frames_prune
    c  8 contexts: one velo_frames_prune_batch against eight velo_frames_prune calls
Every repetition first restores the frame (put + rows), builds the visual set and gates it (velo_build_visual); only the prune is
inside the clock.  5 warm-up repetitions, then median / min / max of --reps.
Kernel time: a run of this tool under `rocprofv3 --kernel-trace --stats` for modes b and c (--no-kernels leaves it out).  Needs a GPU.
Usage: python tools/frame_prune_bench.py [--rows 3000] [--reps 50] [--out profiles/r16_frame_prune.txt]"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import velo_amd  # noqa: E402,F401
from velo_amd import api  # noqa: E402


def make_frames(rng, n):
    """frame1: one camera of n keypoints, all with a depth point; frame2: every second one of them, unchanged"""
    ids = rng.permutation(4 * n)[:n].astype(np.int32)
    kps = (rng.normal(size=(n, 2)) * 0.3).astype(np.float32)
    has = rng.permutation(n).astype(np.int32)
    cloud = (rng.normal(size=(n, 3)) * 5 + [0, 0, 20]).astype(np.float32)
    rows = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    half = np.arange(0, n, 2)
    cloud2 = cloud[has[half]]
    return (ids, kps, has, cloud), rows, (ids[half], kps[half], np.arange(len(half), dtype=np.int32), cloud2), rows[half]


def host_prune(cam, rows, first):
    """velo.h:282-326 for one camera, vectorised"""
    ids, kps, has, cloud = cam
    kept = np.unique(first)
    old = has[kept]
    wd = old != -1
    new_has = np.full(len(kept), -1, dtype=np.int32)
    new_has[wd] = np.arange(int(wd.sum()), dtype=np.int32)
    return (ids[kept], kps[kept], new_has, cloud[old[wd]]), rows[kept]


def clock(prepare, fn, reps):
    t = []
    for k in range(5 + reps):
        prepare()
        t0 = time.perf_counter()
        fn()
        if k >= 5:
            t.append((time.perf_counter() - t0) * 1e6)
    return f"median {np.median(t):.1f} us min {min(t):.1f} max {max(t):.1f}"


def run(args):
    rng = np.random.default_rng(0)
    ct = np.float32([[0, 0, 0], [-.54, 0, 0]])
    n, n_ctx = args.rows, 8
    cams = [make_frames(rng, n) for _ in range(2)]
    ctxs = [api.Context(0) for _ in range(n_ctx)]
    x0 = np.zeros(6)
    for c in ctxs:
        c.frames_reset(ct, arena_capacity=8 << 20)
        for cam, (_, _, f2, r2) in enumerate(cams):
            c.frames_put(0, cam, *f2)
            c.frames_put_descriptors(0, cam, r2)

    def restore(group):
        for c in group:
            for cam, (f1, r1, _, _) in enumerate(cams):
                c.frames_put(1, cam, *f1)
                c.frames_put_descriptors(1, cam, r1)
            c.build_matches(1, 0)
            c.build_visual(x0, 1)
            c.synchronize()
    c0 = ctxs[0]

    def prune_a():
        gm = c0.good_matches()
        for cam, (f1, r1, _, _) in enumerate(cams):
            kp, rows = host_prune(f1, r1, gm["point1"][gm["cam"] == cam])
            c0.frames_put(1, cam, *kp)
            c0.frames_put_descriptors(1, cam, rows)
        c0.synchronize()

    def synced(fn, group):
        def go():
            fn()
            for c in group:
                c.synchronize()                                          # the copies over the blocks are queued behind the call
        return go
    modes = {
        "a (good_matches + host prune + frames_put + frames_put_descriptors)": ([c0], prune_a),
        "b (frames_prune)": ([c0], synced(lambda: c0.frames_prune(1), [c0])),
        "c 8 contexts, eight single calls": (ctxs, synced(lambda: [c.frames_prune(1) for c in ctxs], ctxs)),
        "c 8 contexts, one batch call": (ctxs, synced(lambda: api.frames_prune_batch(ctxs, [1] * n_ctx, raw=True), ctxs)),
    }
    lines = []
    for name, (group, fn) in modes.items():
        if args.only and args.only not in name:
            continue
        lines.append(f"host {name}: {clock(lambda: restore(group), fn, args.reps)}")
        print(lines[-1], flush=True)
    restore([c0])
    kept, _ = c0.frames_prune(1)
    lines.append(f"kept per camera: {[len(k) for k in kept]} of {n}")
    for c in ctxs:
        c.close()
    return lines


def kernel_stats(trace_dir):
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "fr_mark" in r["Name"] or "fr_prune" in r["Name"]:
                    out[r["Name"].split("(")[0].replace("velo::", "")] = (int(r["Calls"]), round(float(r["AverageNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"prune of one frame at 2 cameras x {args.rows} keypoints with rows, about half kept",
             f"host us per prune (5 warm-up repetitions, then {args.reps}); kernel us = average per launch (rocprofv3 --kernel-trace --stats)"]
    lines += run(args)
    if not args.no_kernels and not args.only and shutil.which("rocprofv3"):
        with tempfile.TemporaryDirectory() as td:
            for only in ("b (frames_prune)", "one batch call"):
                tdir = os.path.join(td, only.replace(" ", "_").replace("(", "").replace(")", ""))
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--", sys.executable,
                                os.path.abspath(__file__), "--rows", str(args.rows), "--reps", str(args.reps), "--only", only],
                               check=True, capture_output=True, text=True, timeout=300)
                k = kernel_stats(tdir)
                lines.append(f"kernels {only}: " + (" ".join(f"{a}={c}x{u}us" for a, (c, u) in sorted(k.items())) if k else "no trace found"))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
