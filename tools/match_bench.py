#!/usr/bin/env python3
"""Descriptor matching (velo_match_descriptors, matchFeatures velo.h:499-560) per call, for the three shapes of the reference's loop:
    single   1 job of 3,000 x 3,000                       (one camera of one matchFeatures call)
    frame    2 jobs of 3,000 x 3,000                      (matchFeatures(descriptors, frame1, frame2, matches): both cameras)
    closure  64 jobs: both cameras x 32 loop-closure candidates, one shared query set per camera (main.cpp:351-364)
Needs a GPU (it fails without one: there is no CPU path).  Per shape: us per call (median of --iters synchronous calls after --warmup
calls; a host clock around a call that ends in a device synchronise), bytes moved (the distinct rows up, the outputs down), pair count,
achieved pair-ops/s (512 bits x 2 ops per pair) against the bound of the path used, and the numpy restatement's CPU time
(tests/descriptor_ref.py, one run).  --variant valu runs the diagnostics build's XOR + popcount form instead of the int8-MFMA product.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--no-ref keeps that run short).
Usage: python tools/match_bench.py [--iters 50] [--warmup 5] [--variant mfma|valu] [--shape single|frame|closure] [--no-ref] [--json out.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

MFMA_OPS = 5.0e15        # int8 MFMA, dense: 2x the BF16 rate (~2.5 PF) -- MI355X spec
VALU_LANE_OPS = 39e12    # 32-bit VALU lane-ops/s (256 CUs x 4 SIMD x 16 lanes x 2.4 GHz)
VALU_OPS_PER_PAIR = 32   # 8 x (xor, popcount on two halves, add) per 512-bit pair
HBM = 6.3e12             # bytes/s, measured float4 copy


def shapes(rng):
    n = 3000
    cams = [rng.integers(0, 256, (n, 64), dtype=np.uint8) for _ in range(2)]
    single = [(cams[0], rng.integers(0, 256, (n, 64), dtype=np.uint8))]
    frame = [(cams[c], rng.integers(0, 256, (n, 64), dtype=np.uint8)) for c in range(2)]
    closure = [(cams[c], rng.integers(0, 256, (n, 64), dtype=np.uint8)) for _ in range(32) for c in range(2)]
    return {"single": single, "frame": frame, "closure": closure}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--variant", choices=("mfma", "valu"), default="mfma")
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--shape", choices=("single", "frame", "closure"), default=None, help="one shape only (the profiled runs)")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("match_bench: no GPU visible (/dev/kfd missing); this tool measures the device and has no CPU path")
    try:
        import torch  # noqa: F401  (same library load order as bench.py and the tests)
    except Exception:
        pass
    import velo_amd  # noqa: F401
    from velo_amd import api
    import descriptor_ref as R
    if a.variant == "valu":
        os.environ["VELO_MATCH_VARIANT"] = "0"
        ctx = api.Context(0, lib=api.load_diagnostics_library())
    else:
        ctx = api.Context(0)
    rng = np.random.default_rng(0)
    out = {"variant": a.variant, "iters": a.iters, "warmup": a.warmup, "shapes": {}}
    for name, jobs in shapes(rng).items():
        if a.shape and name != a.shape:
            continue
        got = ctx.match_descriptor_jobs(jobs)                  # the result checked below; counts as warm-up
        for _ in range(a.warmup):
            ctx.match_descriptor_jobs(jobs)
        ts = []
        for _ in range(a.iters):
            t0 = time.perf_counter()
            ctx.match_descriptor_jobs(jobs)
            ts.append(time.perf_counter() - t0)
        us = statistics.median(ts) * 1e6
        pairs = sum(len(q) * len(t) for q, t in jobs)
        distinct = {id(x): len(x) for job in jobs for x in job}
        nq = sum(len(q) for q, _ in jobs)
        up = 64 * sum(distinct.values()) + 32 * len(jobs)
        down = 16 * nq + 8 * len(jobs)
        ops = pairs * 512 * 2
        bound_s = (ops / MFMA_OPS) if a.variant == "mfma" else (pairs * VALU_OPS_PER_PAIR / VALU_LANE_OPS)
        rec = {"jobs": len(jobs), "pairs": pairs, "us_per_call": round(us, 1), "us_min": round(min(ts) * 1e6, 1),
               "bytes_up": up, "bytes_down": down, "pair_ops_per_s": ops / (us * 1e-6),
               "compute_bound_us": round(bound_s * 1e6, 2), "hbm_bound_us": round((up + down) / HBM * 1e6, 2),
               "call_share_of_compute_bound": round(bound_s / (us * 1e-6), 4)}
        if not a.no_ref:
            t0 = time.perf_counter()
            want = R.match_jobs(jobs)
            rec["numpy_ref_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["equal_to_ref"] = bool(all(np.array_equal(got[0][j], want[0][j]) and np.array_equal(got[1][j], want[1][j])
                                           and int(got[2][j]) == int(want[2][j]) and np.array_equal(got[3][j], want[3][j])
                                           for j in range(len(jobs))))
        out["shapes"][name] = rec
        print(f"{name:8s} jobs {len(jobs):3d}  pairs {pairs:.3e}  {us:9.1f} us/call (min {min(ts) * 1e6:.1f})  "
              f"{ops / (us * 1e-6) / 1e12:8.1f} Tpair-op/s  bound {bound_s * 1e6:.2f} us ({a.variant}) / hbm {(up + down) / HBM * 1e6:.2f} us  "
              f"up {up / 1e6:.2f} MB down {down / 1e6:.2f} MB" + (f"  numpy {rec['numpy_ref_ms']:.0f} ms equal={rec['equal_to_ref']}" if not a.no_ref else ""),
              flush=True)
    ctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
