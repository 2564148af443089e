#!/usr/bin/env python3
"""The map hand-over of one scan-to-map odometry step: a window of 17 scans x 120,000 points becomes a context's
target in the newest pose's frame, through
    a  the way without a resident map: every scan of the window moved into the new frame on the host (numpy, vectorised, in double),
       concatenated, and pushed through velo_set_target -- 2,000,000 points over the bus per step
    b  velo_map_insert (the scan just registered, which is the context's source already; the oldest scan leaves) + velo_map_load
    c  8 drives: eight velo_map_load calls against one velo_map_load_batch
The clock is the host's around the call(s) plus a stream synchronisation; 5 warm-up repetitions, then median / min / max of --reps.
(a) is flattered: its transform is one vectorised numpy expression per scan, not a per-point loop.
Kernel time: a run of this tool under `rocprofv3 --kernel-trace --stats` for mode b (--no-kernels leaves it out).  Needs a GPU.
Usage: python tools/scan_map_bench.py [--scans 17] [--reps 50] [--out profiles/r18_scan_map.txt]"""
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

KERNELS = ("map_materialise", "target_ingest", "grid_", "scan_lookback", "bbox", "dimg")


def clock(fn, sync, reps):
    t = []
    for k in range(5 + reps):
        sync()
        t0 = time.perf_counter()
        fn(k)
        sync()
        if k >= 5:
            t.append((time.perf_counter() - t0) * 1e6)
    return f"median {np.median(t):.1f} us min {min(t):.1f} max {max(t):.1f}"


def run(args):
    n_scans, n_drives = args.scans, 8
    plan = synth.drive_plan(n_scans + 1)
    Cm = synth.VELO_TO_CAM.astype(np.float64)
    poses = [Cm @ P @ np.linalg.inv(Cm) for P in plan["poses_velo"]]
    frames = []
    for k in range(n_scans + 1):
        xyz, off = synth.drive_frame(plan, k, n_beams=args.beams, n_azimuth=args.azimuth)
        frames.append((np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3]), np.asarray(off, np.int32)))
    points = sum(len(f[0]) for f in frames[:n_scans])
    ref_inv = np.linalg.inv(poses[n_scans])
    ctxs = [api.Context(0) for _ in range(n_drives)]
    maps = [api.ScanMap(0, n_scans, 1 << 22) for _ in range(n_drives)]
    for c, m in zip(ctxs, maps):
        for k in range(n_scans):
            c.set_source(*frames[k])
            m.insert(c, False, k, poses[k])
        c.set_source(*frames[n_scans])                                  # the scan the step has just registered: resident as the source
    c0, m0 = ctxs[0], maps[0]
    window = [(frames[k][0], frames[k][1], poses[k]) for k in range(n_scans)]

    def host_way(k):
        clouds, offs, at = [], [np.zeros(1, np.int64)], 0
        for xyz, off, pose in window:
            M = ref_inv @ pose
            clouds.append((xyz.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32))
            offs.append(off[1:].astype(np.int64) + at)
            at += len(xyz)
        c0.set_target(np.concatenate(clouds), np.concatenate(offs).astype(np.int32))

    def resident_way(k):
        m0.insert(c0, False, n_scans + k, poses[n_scans])               # the oldest scan leaves
        m0.load(c0, ref_inv)

    def sync_all():
        for c in ctxs:
            c.synchronize()
    invs = [ref_inv] * n_drives
    modes = {
        "a (numpy transform of the window + velo_set_target)": (host_way, c0.synchronize),
        "b (velo_map_insert + velo_map_load)": (resident_way, c0.synchronize),
        "c 8 drives, eight velo_map_load calls": (lambda k: [m.load(c, ref_inv) for m, c in zip(maps, ctxs)], sync_all),
        "c 8 drives, one velo_map_load_batch": (lambda k: api.map_load_batch(maps, ctxs, invs), sync_all),
    }
    lines = [f"window: {n_scans} scans, {points} points, {sum(len(f[1]) - 1 for f in frames[:n_scans])} rings"]
    for name, (fn, sync) in modes.items():
        if args.only and args.only not in name:
            continue
        lines.append(f"host {name}: {clock(fn, sync, args.reps)}")
        print(lines[-1], flush=True)
    if not args.only:
        info = m0.info()
        lines.append(f"map after the run: {info['scans']} scans, {info['points']} points, arena {info['arena_points']} points after {info['arena_growths']} growths, "
                     f"{info['evictions']} evictions")
    for m in maps:
        m.close()
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
    ap.add_argument("--scans", type=int, default=17)
    ap.add_argument("--beams", type=int, default=synth.N_BEAMS)
    ap.add_argument("--azimuth", type=int, default=synth.N_AZIMUTH)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"the map hand-over of one scan-to-map step, {args.scans} scans of {args.beams} x {args.azimuth} beams x azimuths, all in the newest pose's frame",
             f"host us per step, call(s) + stream synchronisation (5 warm-up repetitions, then {args.reps}); kernel us = average per launch (rocprofv3 --kernel-trace --stats)",
             "(a) is flattered: its transform is vectorised numpy"]
    lines += run(args)
    if not args.no_kernels and not args.only and shutil.which("rocprofv3"):
        with tempfile.TemporaryDirectory() as td:
            only = "b (velo_map_insert"
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td, "--", sys.executable,
                            os.path.abspath(__file__), "--scans", str(args.scans), "--beams", str(args.beams), "--azimuth", str(args.azimuth),
                            "--reps", str(args.reps), "--only", only], check=True, capture_output=True, text=True, timeout=400)
            k = kernel_stats(td)
            lines.append("kernels b: " + (" ".join(f"{a}={c}x{u}us" for a, (c, u) in sorted(k.items())) if k else "no trace found"))
            print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
