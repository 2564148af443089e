#!/usr/bin/env python3
"""The visual set of one loop-closure edge and the screening of a frame's candidates: host time per call at
2 cameras x 3,000 x 3,000 descriptor rows (queries = near-duplicates of train rows, 0-40 flipped bits, so the filter keeps and
drops), through
    a  the path before the resident rows: velo_match_descriptors from host rows, the records gathered on the host (vectorised numpy
       over the kept pairs -- cheaper than the adaptor's walk through four nested containers, so (a) is flattered), velo_set_visual;
       screening: one velo_match_descriptors call of n_cand x 2 jobs (the shared query set travels once)
    b  velo_build_matches_desc on resident rows; screening: velo_match_frames
    c  8 contexts: one velo_build_matches_desc_batch against eight velo_build_matches_desc calls
Host time: a clock around the call, which ends in a device synchronisation; 5 warm-up calls, then median / min / max of --reps calls.
Kernel time: a run of this tool under `rocprofv3 --kernel-trace --stats` for modes b and c (--no-kernels leaves it out).  Needs a GPU.
The claims to test: b beats a; the resident screening approaches the kernel time; c beats eight single calls.
Usage: python tools/loop_matches_bench.py [--rows 3000] [--cand 32] [--reps 100] [--out profiles/r14_loop_matches.txt]"""
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


def make_frame(rng, n, base=None):
    """one camera: (ids, keypoints, has_depth, cloud), rows; rows = near-duplicates of `base` when given"""
    ids = rng.permutation(4 * n)[:n].astype(np.int32)
    kps = (rng.normal(size=(n, 2)) * 0.3).astype(np.float32)
    with_depth = np.flatnonzero(rng.random(n) < 0.5)
    has = np.full(n, -1, dtype=np.int32)
    has[with_depth] = rng.permutation(len(with_depth)).astype(np.int32)
    cloud = (rng.normal(size=(len(with_depth), 3)) * 5 + [0, 0, 20]).astype(np.float32)
    if base is None:
        rows = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    else:
        bits = np.unpackbits(base[rng.permutation(len(base))[:n]], axis=1, bitorder="little")
        flip = rng.random(bits.shape) < (rng.integers(0, 41, (n, 1)) / 512.0)
        rows = np.packbits(bits ^ flip.astype(np.uint8), axis=1, bitorder="little")
    return (ids, kps, has, cloud), rows


def host_records(f1, f2, pairs_per_cam, cam_trans):
    """velo.h:627-654 without landmarks, vectorised over the kept pairs"""
    parts = []
    for cam, pairs in enumerate(pairs_per_cam):
        (_, kp1, has1, cl1), (_, kp2, has2, cl2) = f1[cam], f2[cam]
        p1, p2 = pairs[:, 0], pairs[:, 1]
        out = np.zeros(len(pairs), dtype=api.MATCH_DTYPE)
        h1, h2 = has1[p1], has2[p2]
        out["p3_1"][h1 != -1] = cl1[h1[h1 != -1]]
        out["p3_2"][h2 != -1] = cl2[h2[h2 != -1]]
        out["p2_1"], out["p2_2"], out["t_cam"] = kp1[p1], kp2[p2], cam_trans[cam]
        out["cam"], out["point1"], out["point2"], out["d1"], out["d2"] = cam, p1, p2, h1 != -1, h2 != -1
        parts.append(out)
    return np.concatenate(parts)


def clock(fn, reps):
    for _ in range(5):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return f"median {np.median(t):.1f} us min {min(t):.1f} max {max(t):.1f}"


def run(args):
    rng = np.random.default_rng(0)
    ct = np.float32([[0, 0, 0], [-.54, 0, 0]])
    n, n_ctx = args.rows, 8
    train = [make_frame(rng, n) for _ in range(2)]
    query = [make_frame(rng, n, base=train[cam][1]) for cam in range(2)]
    cands = [[make_frame(rng, n) for _ in range(2)] for _ in range(args.cand - 1)] + [train]
    ctxs = [api.Context(0) for _ in range(n_ctx)]
    for c in ctxs:
        c.frames_reset(ct, arena_capacity=64 * n * 2 * (args.cand + 2))
        for f, fr in enumerate([query] + cands):
            for cam, (kp, rows) in enumerate(fr):
                c.frames_put(f, cam, *kp)
                c.frames_put_descriptors(f, cam, rows)
    c0 = ctxs[0]
    f1, f2 = [q[0] for q in query], [t[0] for t in train]
    lines = []

    def edge_a():
        _, _, _, pairs = c0.match_descriptor_jobs([(query[cam][1], train[cam][1]) for cam in range(2)], args.thresh)
        c0.set_visual(host_records(f1, f2, pairs, ct))
        c0.synchronize()
    jobs_a = [(query[cam][1], cd[cam][1]) for cd in cands for cam in range(2)]
    frames2 = list(range(1, args.cand + 1))
    modes = {
        "edge a (match_descriptors + host records + set_visual)": edge_a,
        "edge b (build_matches_desc)": lambda: c0.build_matches_desc(0, args.cand, None, args.thresh),
        f"screen a ({args.cand} candidates, match_descriptors)": lambda: c0.match_descriptor_jobs(jobs_a, args.thresh),
        f"screen b ({args.cand} candidates, match_frames)": lambda: c0.match_frames(0, frames2, args.thresh),
        "edge c 8 contexts, eight single calls": lambda: [c.build_matches_desc(0, args.cand, None, args.thresh) for c in ctxs],
        "edge c 8 contexts, one batch call": lambda: api.build_matches_desc_batch(ctxs, [0] * n_ctx, [args.cand] * n_ctx, None, args.thresh),
    }
    for name, fn in modes.items():
        if args.only and args.only not in name:
            continue
        lines.append(f"host {name}: {clock(fn, args.reps)}")
        print(lines[-1], flush=True)
    kept = c0.build_matches_desc(0, args.cand, None, args.thresh)[0]
    lines.append(f"kept per camera on the edge: {kept.tolist()} of {n}")
    for c in ctxs:
        c.close()
    return lines


def kernel_stats(trace_dir):
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                if "match_" in r["Name"] or "fr_emit" in r["Name"]:
                    out[r["Name"].split("(")[0].replace("velo::", "")] = (int(r["Calls"]), round(float(r["AverageNs"]) / 1e3, 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3000)
    ap.add_argument("--cand", type=int, default=32)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--thresh", type=float, default=29.0)
    ap.add_argument("--only", default="")
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = [f"one loop-closure edge at 2 cameras x {args.rows} x {args.rows} rows; screening of {args.cand} candidates",
             f"host us per call (5 warm-up calls, then {args.reps}); kernel us = average per launch (rocprofv3 --kernel-trace --stats)"]
    lines += run(args)
    if not args.no_kernels and not args.only and shutil.which("rocprofv3"):
        with tempfile.TemporaryDirectory() as td:
            for only in ("edge b", "screen b", "one batch call"):
                tdir = os.path.join(td, only.replace(" ", "_"))
                subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--", sys.executable,
                                os.path.abspath(__file__), "--rows", str(args.rows), "--cand", str(args.cand), "--reps", str(args.reps),
                                "--thresh", str(args.thresh), "--only", only], check=True, capture_output=True, text=True, timeout=600)
                k = kernel_stats(tdir)
                lines.append(f"kernels {only}: " + (" ".join(f"{a}={c}x{u}us" for a, (c, u) in sorted(k.items())) if k else "no trace found"))
                print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
