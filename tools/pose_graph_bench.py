#!/usr/bin/env python3
"""Batch optimisation of a drive's pose graph: the host time of one velo_graph_optimize call, of one of its LM
iterations and of one of its CG iterations, on a synthetic drive of the size of KITTI 00: 4,541 poses about 0.8 m apart on a circle of 3,000
frames (5 mrad / 10 cm of jitter per pose), so that the last 1,541 frames drive over the first ones again.  Edges: odometry for dframe = 1 .. 4 (noise
1 mrad / 2 cm), and loop edges chosen by the reference's rule -- for every frame the candidates frame - k, k = 10 ba_every,
11 ba_every, ... (main.cpp:157-158), kept when the relative translation with its y divided by 20 is within loop_close_thresh = 10 m
(main.cpp:328-341) -- measured with a tenth of the noise at info 1.  The start is the dead reckoning of the dframe = 1 edges.

Every repetition rebuilds the store (a call moves the poses); only the optimize call is timed, and it ends in a device
synchronisation.  Beside it: the same problem solved by the numpy restatement's sparse `direct` solver (tests/pose_graph_ref.py,
SuperLU on the damped normal equations) on the host -- its whole time, dominated by the restatement's per-edge Python loop, and the
time inside the linear solver alone, which is the figure to hold against the CG.  --solver envelope adds a line for the envelope solver
(linear_solver="envelope": the exact Cholesky in reverse Cuthill-McKee order) beside the CG lines; --cg-tol with no value leaves the CG
lines out.  Nothing gates on this tool.
Usage: python tools/pose_graph_bench.py [--reps 5] [--cg-tol 1e-10 1e-4] [--cg-max 2000] [--long-cap 10000] [--solver envelope] [--no-host] [--no-gpu] [--out profiles/r20_pose_graph.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import velo_amd  # noqa: E402,F401
import pose_graph_ref as G  # noqa: E402

N, LAP, BA_EVERY, LOOP_CLOSE_THRESH = 4541, 3000, 10, 10.0


def make_drive(seed=20):
    rng = np.random.default_rng(seed)
    radius = LAP * 0.8 / (2.0 * np.pi)
    truth = []
    for i in range(N):                                                 # heading about the camera's y axis, forward along its z
        a = 2.0 * np.pi * i / LAP
        T = G.pose_mat(np.array([0.0, a, 0.0, radius * (1.0 - np.cos(a)), 0.0, radius * np.sin(a)]))
        truth.append(G.pose_vec(T @ G.pose_mat(np.concatenate([5e-3 * rng.normal(size=3), 0.1 * rng.normal(size=3)]))))
    mats = [G.pose_mat(x) for x in truth]
    inv = [np.linalg.inv(T) for T in mats]

    def measure(a, b, scale):
        z = G.pose_vec(inv[a] @ mats[b])
        return G.compose(z, np.concatenate([scale * 1e-3 * rng.normal(size=3), scale * 0.02 * rng.normal(size=3)]))
    edges = [(i, i + d, measure(i, i + d, 1.0), 1.0) for d in (1, 2, 3, 4) for i in range(N - d)]
    n_odometry = len(edges)
    for frame in range(N):
        for k in range(10 * BA_EVERY, frame + 1, BA_EVERY):
            t = (inv[frame - k] @ mats[frame])[:3, 3].copy()
            t[1] /= 20.0
            if np.linalg.norm(t) <= LOOP_CLOSE_THRESH:
                edges.append((frame - k, frame, measure(frame - k, frame, 0.1), 1.0))
    poses = G._dead_reckoning(truth[0], [e[2] for e in edges[:N - 1]])
    return dict(poses={i: p for i, p in enumerate(poses)}, edges=edges, fixed=[0], truth=truth, n_odometry=n_odometry)


def med(v):
    v = np.sort(np.asarray(v, dtype=np.float64))
    return f"{np.median(v):.2f} [{v[0]:.2f}-{v[-1]:.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cg-tol", type=float, nargs="*", default=[1e-10, 1e-4])
    ap.add_argument("--cg-max", type=int, default=2000)
    ap.add_argument("--long-cap", type=int, default=10000, help="one more run of the last tolerance with this cap on the CG iterations (0: none)")
    ap.add_argument("--solver", choices=["envelope"], default=None, help="one more line: the same drive with this linear solver")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = make_drive()
    truth = np.array(g["truth"])
    start = np.array([g["poses"][i] for i in range(N)])
    lines = [f"pose graph: {N} poses, {g['n_odometry']} odometry edges (dframe 1..4), {len(g['edges']) - g['n_odometry']} loop edges; "
             f"largest position error of the start {np.linalg.norm(start[:, 3:] - truth[:, 3:], axis=1).max():.1f} m"]
    if not a.no_gpu:
        from velo_amd import api
        frm, to = [e[0] for e in g["edges"]], [e[1] for e in g["edges"]]
        z, info = np.array([e[2] for e in g["edges"]]), [e[3] for e in g["edges"]]
        ctx = api.Context(0)
        configs = [(tol, a.cg_max, a.reps) for tol in a.cg_tol]
        if a.cg_tol and a.long_cap > a.cg_max:
            configs.append((a.cg_tol[-1], a.long_cap, 1))
        for tol, cap, reps in configs:
            ms, s, out = [], None, None
            for rep in range(reps + 1):
                ctx.graph_reset(len(frm))
                ctx.graph_set_poses(0, start)
                ctx.graph_add_edges(frm, to, z, info)
                ctx.synchronize()
                t0 = time.perf_counter()
                s = ctx.graph_optimize(g["fixed"], cg_tolerance=tol, cg_max_iterations=cap)
                if rep > 0:
                    ms.append(1e3 * (time.perf_counter() - t0))
            out = ctx.graph_get_poses(0, N)
            cg = [s.trace[i].cg_iterations for i in range(s.n_trace)]
            t = float(np.median(ms))
            lines.append(f"GPU  cg_tolerance {tol:g}, cap {cap}: optimize {med(ms)} ms; {s.iterations} LM iterations ({t / max(s.iterations, 1):.2f} ms each), "
                         f"{sum(cg)} CG iterations ({1e3 * t / max(sum(cg), 1):.1f} us each, everything else included), per LM iteration {cg}; "
                         f"termination {s.termination}, cost {s.initial_cost:.4e} -> {s.final_cost:.4e}, largest position error {np.linalg.norm(out[:, 3:] - truth[:, 3:], axis=1).max():.2f} m")
        if a.solver == "envelope":
            ms, s = [], None
            for rep in range(a.reps + 1):
                ctx.graph_reset(len(frm))
                ctx.graph_set_poses(0, start)
                ctx.graph_add_edges(frm, to, z, info)
                ctx.synchronize()
                t0 = time.perf_counter()
                s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
                if rep > 0:
                    ms.append(1e3 * (time.perf_counter() - t0))
            out = ctx.graph_get_poses(0, N)
            gi = ctx.graph_info()
            t = float(np.median(ms))
            prob = G.problem_of(g)
            slot = prob.slot
            pairs = [(slot[e[0]], slot[e[1]]) for e in g["edges"] if e[0] in slot and e[1] in slot]
            work = api.graph_order(prob.n_free, [p[0] for p in pairs], [p[1] for p in pairs])[2]["work"]
            lines.append(f"GPU  envelope solver: optimize {med(ms)} ms; {s.iterations} LM iterations ({t / max(s.iterations, 1):.2f} ms each); "
                         f"termination {s.termination}, cost {s.initial_cost:.4e} -> {s.final_cost:.4e}, largest position error {np.linalg.norm(out[:, 3:] - truth[:, 3:], axis=1).max():.2f} m; "
                         f"widest row {gi['envelope_widest_row']} blocks, envelope {gi['envelope_blocks']} blocks, work {work} block products per factorisation")
        ctx.close()
    if not a.no_host:
        prob = G.problem_of(g)
        t0 = time.perf_counter()
        w = G.solve(prob, "direct")
        t = time.perf_counter() - t0
        x = w["x"].reshape(-1, 6)
        lines.append(f"host restatement, sparse direct: {1e3 * t:.0f} ms in all, {1e3 * w['linear_seconds']:.0f} ms inside the linear solver "
                     f"({1e3 * w['linear_seconds'] / max(w['iterations'], 1):.1f} ms per LM iteration); {w['iterations']} LM iterations, termination {w['termination']}, "
                     f"cost {w['initial_cost']:.4e} -> {w['final_cost']:.4e}, largest position error {np.linalg.norm(x[:, 3:] - truth[1:, 3:], axis=1).max():.2f} m")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
