#!/usr/bin/env python3
"""A frame put with its keypoint depth: host time per frame at 2 cameras x 3,000 keypoints with descriptor rows
on the 120,000-point street scan, the landmark log appended as well, through
    a  the four calls per camera: velo_project_lidar, velo_depth_association, velo_frames_put + velo_frames_put_descriptors,
       velo_landmarks_observe -- has_depth and the depth cloud come to the host once and go back twice
    b  velo_frames_put_frame with VELO_PUT_OBSERVE
    c  8 contexts: one velo_frames_put_frame_batch against eight velo_frames_put_frame calls
The clock is the host's around the call(s) plus a stream synchronisation.  Every repetition puts a NEW frame (a frame is observed
once) after the one before has been dropped, so the arenas are in their steady state; the log is sized for the whole run.
5 warm-up repetitions, then median / min / max of --reps.
Kernel time: a run of this tool under `rocprofv3 --kernel-trace --stats` for modes a and b (--no-kernels leaves it out).  Needs a GPU.
Usage: python tools/frame_depth_bench.py [--rows 3000] [--reps 50] [--out profiles/r17_frame_depth.txt]"""
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
from velo_amd import api, synth  # noqa: E402

KERNELS = ("fr_depth", "project_ring", "depth_assoc", "depth_compact", "scan_tiles", "scan_sums", "scan_add", "lm_append")


def clock(prepare, fn, reps):
    t = []
    for k in range(5 + reps):
        prepare(k)
        t0 = time.perf_counter()
        fn(k)
        if k >= 5:
            t.append((time.perf_counter() - t0) * 1e6)
    return f"median {np.median(t):.1f} us min {min(t):.1f} max {max(t):.1f}"


def run(args):
    rng = np.random.default_rng(0)
    ct = np.ascontiguousarray(synth.CAM_TRANS[:2], np.float32)
    w = synth.cam_window()
    n, n_ctx, thresh = args.rows, 8, synth.DEPTH_ASSOC_THRESH
    d = synth.scan_pair()                                               # 64 x 1875
    cams = [api.FrameCam(cam * 4 * n + rng.permutation(4 * n)[:n], synth.keypoints_in_window(n, seed=31 + cam), w,
                         rng.integers(0, 256, (n, 64), dtype=np.uint8)) for cam in range(2)]
    ctxs = [api.Context(0) for _ in range(n_ctx)]
    for c in ctxs:
        c.set_source(d["src_xyz"], d["src_off"])
        c.frames_reset(ct, arena_capacity=8 << 20)
        c.landmarks_reset(ct, log_capacity=2 * n * (4 * (args.reps + 8)))     # every mode appends reps + 5 frames

    def four_calls(c, frame):
        for cam, K in enumerate(cams):
            c.project_lidar(False, ct[cam], K.window)
            kd, has = c.depth_association(K.keypoints_xy, thresh)
            c.frames_put(frame, cam, K.ids, K.keypoints_xy, has, kd)
            c.frames_put_descriptors(frame, cam, K.rows)
            c.landmarks_observe(frame, cam, K.ids, K.keypoints_xy, has, kd)
    frame0 = [0]

    def mode(group, fn):
        base = frame0[0]
        frame0[0] += 5 + args.reps + 1

        def prepare(k):
            for c in group:
                if k > 0:
                    c.frames_drop(base + k - 1)
                c.synchronize()

        def go(k):
            fn(base + k)
            for c in group:
                c.synchronize()                                          # the copies into the blocks are queued behind the call
        return prepare, go
    c0 = ctxs[0]
    modes = {
        "a (project_lidar + depth_association + frames_put + frames_put_descriptors + landmarks_observe, per camera)":
            ([c0], lambda f: four_calls(c0, f)),
        "b (frames_put_frame, VELO_PUT_OBSERVE)": ([c0], lambda f: c0.frames_put_frame(f, cams, thresh, observe=True)),
        "c 8 contexts, eight single calls": (ctxs, lambda f: [c.frames_put_frame(f, cams, thresh, observe=True) for c in ctxs]),
        "c 8 contexts, one batch call": (ctxs, lambda f: api.frames_put_frame_batch(ctxs, [f] * n_ctx, [cams] * n_ctx, thresh, observe=True, raw=True)),
    }
    lines = []
    for name, (group, fn) in modes.items():
        if args.only and args.only not in name:
            continue
        lines.append(f"host {name}: {clock(*mode(group, fn), args.reps)}")
        print(lines[-1], flush=True)
    if not args.only:                                                   # (a traced run holds the kernels of its mode only)
        n_wd = c0.frames_put_frame(frame0[0], cams, thresh)
        lines.append(f"keypoints with depth per camera: {n_wd.tolist()} of {n}")
    for c in ctxs:
        c.close()
    return lines


def kernel_stats(trace_dir):
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if any(k in r["Name"] for k in KERNELS):
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
    lines = [f"one frame at 2 cameras x {args.rows} keypoints with rows on the 120,000-point street scan, depth threshold {synth.DEPTH_ASSOC_THRESH}, landmark log appended",
             f"host us per frame, call(s) + stream synchronisation (5 warm-up repetitions, then {args.reps}); kernel us = average per launch (rocprofv3 --kernel-trace --stats)"]
    lines += run(args)
    if not args.no_kernels and not args.only and shutil.which("rocprofv3"):
        with tempfile.TemporaryDirectory() as td:
            for only in ("a (project_lidar", "b (frames_put_frame"):
                tdir = os.path.join(td, only[0])
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--", sys.executable,
                                os.path.abspath(__file__), "--rows", str(args.rows), "--reps", str(args.reps), "--only", only],
                               check=True, capture_output=True, text=True, timeout=300)
                k = kernel_stats(tdir)
                lines.append(f"kernels {only[0]}: " + (" ".join(f"{a}={c}x{u}us" for a, (c, u) in sorted(k.items())) if k else "no trace found"))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
