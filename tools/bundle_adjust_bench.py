#!/usr/bin/env python3
"""Bundle adjustment of a window over the resident landmark store: the host time of one velo_landmarks_adjust call
and of one of its LM iterations, for a window of 1 fixed + 10 free frames, 2 cameras and 3,000 / 6,000 landmarks that live through the
whole window (each camera sees a landmark with probability 0.8, 40 % of the observations carry LiDAR depth).  The free poses start
3 cm / 2 mrad off, the points are triangulated with those poses.  Every repetition rebuilds the store (a call moves poses and points,
so a second call on the same store would start at the minimum); only the adjust call is timed, and it ends in a device
synchronisation.  50 repetitions after 5 warm-up ones, median [min-max].  Kernel share: a run of its own under
`rocprofv3 --kernel-trace --stats` of a few repetitions (--no-kernels leaves it out).  Needs a GPU.
Usage: python tools/bundle_adjust_bench.py [--landmarks 3000 6000] [--reps 50] [--warmup 5] [--out profiles/r19_bundle_adjust.txt]"""
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

N_FRAMES, N_CAMS = 11, 2


def make_window(n_ids, seed=19):
    rng = np.random.default_rng(seed)
    k = np.arange(N_FRAMES, dtype=np.float64)
    poses = np.stack([0.002 * np.sin(0.7 * k), 0.004 * k, 0.001 * np.cos(0.5 * k), 0.02 * k, 0.01 * np.sin(k), 0.3 * k], axis=1)
    poses[0] = 0.0
    z = 6.0 + 40.0 * rng.random(n_ids)
    truth = np.stack([(rng.random(n_ids) - 0.5) * 1.2 * z, (rng.random(n_ids) - 0.5) * 0.4 * z, z + 3.0], axis=1)
    tc = synth.CAM_TRANS[:N_CAMS].astype(np.float64)
    frames = []
    for f in range(N_FRAMES):
        R = synth.rotvec_to_matrix(poses[f, :3])
        M = (truth - poses[f, 3:]) @ R
        per_cam = []
        for cam in range(N_CAMS):
            seen = np.flatnonzero((rng.random(n_ids) < 0.8) & (M[:, 2] > 1.0))
            seen = seen[rng.permutation(len(seen))]
            Mc = M[seen] + tc[cam]
            kp = (Mc[:, :2] / Mc[:, 2:3] + 7e-4 * rng.normal(size=(len(seen), 2))).astype(np.float32)
            depth = rng.random(len(seen)) < 0.4
            has = np.full(len(seen), -1, dtype=np.int32)
            has[depth] = rng.permutation(int(depth.sum())).astype(np.int32)
            cloud = np.zeros((int(depth.sum()), 3), dtype=np.float32)
            cloud[has[depth]] = M[seen[depth]] + 0.03 * rng.normal(size=(int(depth.sum()), 3))
            per_cam.append((seen.astype(np.int32), kp, has, cloud))
        frames.append(per_cam)
    start = poses.copy()
    start[1:, :3] += 2e-3 * rng.normal(size=(N_FRAMES - 1, 3))
    start[1:, 3:] += 0.03 * rng.normal(size=(N_FRAMES - 1, 3))
    return dict(poses=start, cam_trans=synth.CAM_TRANS[:N_CAMS].astype(np.float32).copy(), frames=frames)


def fill(ctx, w):
    ctx.landmarks_reset(w["cam_trans"], log_capacity=1 << 18)
    for f in range(N_FRAMES):
        ctx.landmarks_set_pose(f, w["poses"][f])
    for f, per_cam in enumerate(w["frames"]):
        for cam, (ids, kp, has, cloud) in enumerate(per_cam):
            ctx.landmarks_observe(f, cam, ids, kp, has, cloud)
        ctx.landmarks_triangulate(f)


def measure(n_ids, reps, warmup):
    w = make_window(n_ids)
    ctx = api.Context(0)
    us, its, s = [], [], None
    for r in range(warmup + reps):
        fill(ctx, w)
        t0 = time.perf_counter()
        _, s = ctx.landmarks_adjust(list(range(N_FRAMES)), 1)
        dt = (time.perf_counter() - t0) * 1e6
        if r >= warmup:
            us.append(dt)
            its.append(s.iterations)
    ctx.close()
    us, per = np.array(us), np.array(us) / np.maximum(np.array(its), 1)
    return (f"adjust landmarks={n_ids} taking_part={s.n_landmarks} blocks={s.n_blocks} residuals={s.n_residuals} iterations={s.iterations} "
            f"cost {s.initial_cost:.4g} -> {s.final_cost:.4g}: {np.median(us):.0f} us per call [{us.min():.0f}-{us.max():.0f}], "
            f"{np.median(per):.1f} us per LM iteration [{per.min():.1f}-{per.max():.1f}] ({len(us)} repetitions after {warmup})")


def kernel_share(n_ids, td):
    tdir = os.path.join(td, f"trace_{n_ids}")
    subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--", sys.executable, os.path.abspath(__file__),
                    "--landmarks", str(n_ids), "--reps", "3", "--warmup", "1", "--no-kernels"], check=True, capture_output=True, text=True, timeout=900)
    rows = []
    for path in glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            rows += list(csv.DictReader(f))
    total = {}
    for r in rows:
        name = r["Kernel_Name"].split("(")[0].replace("velo::", "")
        if name.startswith("ba_"):
            t = total.setdefault(name, [0, 0.0])
            t[0] += 1
            t[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    if not total:
        return f"kernels landmarks={n_ids}: no trace found"
    whole = sum(t[1] for t in total.values())
    return f"kernels landmarks={n_ids}: " + ", ".join(f"{k} {100 * t[1] / whole:.0f}% ({t[1] / t[0]:.1f} us x {t[0]})" for k, t in sorted(total.items(), key=lambda kv: -kv[1][1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, nargs="+", default=[3000, 6000])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"bundle adjustment of a window: {N_FRAMES - 1} free + 1 fixed frames, {N_CAMS} cameras; host us around velo_landmarks_adjust (ends in a synchronisation)"]
    for n in args.landmarks:
        lines.append(measure(n, args.reps, args.warmup))
        print(lines[-1], flush=True)
    if not args.no_kernels and shutil.which("rocprofv3"):
        with tempfile.TemporaryDirectory() as td:
            for n in args.landmarks:
                lines.append(kernel_share(n, td))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
