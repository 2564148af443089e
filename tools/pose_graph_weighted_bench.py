#!/usr/bin/env python3
"""The pose graph with matrix information and a robust loss on the drive of tools/pose_graph_bench.py: 4,541 poses,
18,154 odometry and 4,623 loop edges.  Two graphs on the same edges:
  scalar    every edge through velo_graph_add_edges with info 1, as pose_graph_bench.py loads it: graph_linearize_kernel;
  weighted  every edge through velo_graph_add_edges_weighted with the information matched to the noise it was measured with
            (diag(1 / (1 mrad)^2 x 3, 1 / (2 cm)^2 x 3), a hundred times that on the loop edges) and Cauchy(--cauchy) on the loop
            edges: graph_linearize_weighted_kernel.
For each, with the CG and with the envelope solver: the host time of one velo_graph_optimize call (it ends in a device
synchronisation) and of one of its LM iterations, and a SHA-256 of the final poses and the summary, which is how a scalar run is
held against the same run of another build.  The time of one linearise launch is a kernel's and is read from a trace of its own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/pose_graph_weighted_bench.py --reps 1 --solver envelope
A library without the weighted entry (an earlier commit's) runs the scalar lines only.  Nothing gates on this tool.
Usage: python tools/pose_graph_weighted_bench.py [--reps 3] [--solver cg envelope] [--kind scalar weighted] [--cauchy 2.0] [--cg-max 2000] [--out FILE]"""
import argparse
import ctypes as C
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import velo_amd  # noqa: E402,F401
import pose_graph_bench as B  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--solver", nargs="*", default=["cg", "envelope"], choices=["cg", "envelope"])
    ap.add_argument("--kind", nargs="*", default=["scalar", "weighted"], choices=["scalar", "weighted"])
    ap.add_argument("--cauchy", type=float, default=2.0)
    ap.add_argument("--cg-max", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from velo_amd import api
    g = B.make_drive()
    truth = np.array(g["truth"])
    start = np.array([g["poses"][i] for i in range(B.N)])
    frm, to = [e[0] for e in g["edges"]], [e[1] for e in g["edges"]]
    z, info = np.array([e[2] for e in g["edges"]]), [e[3] for e in g["edges"]]
    E, n_odo = len(frm), g["n_odometry"]
    noise = np.array([1.0 / 1e-3 ** 2] * 3 + [1.0 / 0.02 ** 2] * 3)
    W = np.zeros((E, 6, 6))
    W[:, np.arange(6), np.arange(6)] = noise
    W[n_odo:] *= 100.0                                                 # the loop edges were measured with a tenth of the noise
    loss = np.zeros(E)
    loss[n_odo:] = a.cauchy
    lines = [f"pose graph: {B.N} poses, {n_odo} odometry edges (dframe 1..4), {E - n_odo} loop edges; weighted: information matched to the noise, "
             f"Cauchy({a.cauchy:g}) on the loop edges"]
    kinds = [k for k in a.kind if k == "scalar" or hasattr(api.Context, "graph_add_edges_weighted")]
    ctx = api.Context(0)
    for solver in a.solver:
        for kind in kinds:
            ms, s = [], None
            for rep in range(a.reps + 1):
                ctx.graph_reset(E)
                ctx.graph_set_poses(0, start)
                if kind == "scalar":
                    ctx.graph_add_edges(frm, to, z, info)
                else:
                    ctx.graph_add_edges_weighted(frm, to, z, W, loss)
                ctx.synchronize()
                t0 = time.perf_counter()
                s = ctx.graph_optimize(g["fixed"], cg_max_iterations=a.cg_max, linear_solver=solver)
                if rep > 0:
                    ms.append(1e3 * (time.perf_counter() - t0))
            out = ctx.graph_get_poses(0, B.N)
            digest = hashlib.sha256(out.tobytes() + C.string_at(C.addressof(s), C.sizeof(s))).hexdigest()[:16]
            t = float(np.median(ms))
            line = (f"GPU  {kind:8s} {solver:8s}: optimize {B.med(ms)} ms; {s.iterations} LM iterations ({t / max(s.iterations, 1):.2f} ms each), {s.evaluations} evaluations; "
                    f"termination {s.termination}, cost {s.initial_cost:.4e} -> {s.final_cost:.4e}, largest position error "
                    f"{np.linalg.norm(out[:, 3:] - truth[:, 3:], axis=1).max():.2f} m; sha256 of poses and summary {digest}")
            if kind == "weighted":
                weight = ctx.graph_edge_stats()[1]
                line += f"; loop edges' weights: smallest {weight[n_odo:].min():.3f}, median {np.median(weight[n_odo:]):.3f}"
            lines.append(line)
    ctx.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
