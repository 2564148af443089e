#!/usr/bin/env python3
"""Corner detection (velo_detect_features, detectFeatures velo.h:118-177) per call on the resident images, for the reference's shape:
    frame        2 cameras of 1226 x 370, GFTTDetector(3000, 0.001, 12), 1,500 existing points each (one call, two jobs)
    one_camera   the same for camera 0 alone
    md5          both cameras at min_distance = 5 (the cap of 3,000 is reached; most candidates stay undecided longest)
Needs a GPU (it fails without one: there is no CPU path).  Per shape: us per call (median of --iters synchronous calls after --warmup
calls; a host clock around work that ends in a device synchronise), whether the result equals the numpy restatement
(tests/gftt_ref.py), per camera the candidates / corners / selection passes (the diagnostics build's velo_diag_detect_counters: the
passes by the whole device plus those of the single-workgroup loop, and how many candidates that loop still had to decide), and the
restatement's CPU time as a sanity figure.  Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats`
(--no-ref keeps that run short).
Usage: python tools/detect_bench.py [--iters 200] [--warmup 10] [--no-ref] [--json out.json]"""
import argparse
import ctypes as C
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


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts) * 1e6, min(ts) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("detect_bench: no GPU visible (/dev/kfd missing); this tool measures the device and has no CPU path")
    try:
        import torch  # noqa: F401  (same library load order as bench.py and the tests)
    except Exception:
        pass
    import velo_amd  # noqa: F401
    from velo_amd import api, synth
    import gftt_ref as G
    imgs = synth.tracking_frames(1226, 370, seed=0)["next"]
    ex = [synth.tracking_points(1500, seed=5 + c) for c in range(2)]
    shapes = {"frame": ([(0, ex[0]), (1, ex[1])], {}), "one_camera": ([(0, ex[0])], {}),
              "md5": ([(0, ex[0]), (1, ex[1])], {"min_distance": 5.0})}
    out = {"iters": a.iters, "warmup": a.warmup, "shapes": {}}

    diag = api.load_diagnostics_library()
    fn = diag.velo_diag_detect_counters
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    ctx = api.Context(0)
    dctx = api.Context(0, lib=diag)
    for c in (ctx, dctx):
        c.set_images(imgs)

    def upload():
        ctx.set_images(imgs)
        ctx.synchronize()
    us, mn = timed(upload, a.iters, a.warmup)
    out["shapes"]["set_images"] = {"us_per_call": round(us, 1), "us_min": round(mn, 1)}
    print(f"set_images  2 x 1226x370 (for comparison) {us:9.1f} us/call (min {mn:.1f})", flush=True)
    for name, (jobs, params) in shapes.items():
        got = ctx.detect_features_raw(jobs, 3000, **params)
        us, mn = timed(lambda: ctx.detect_features_raw(jobs, 3000, **params), a.iters, a.warmup)
        rec = {"jobs": len(jobs), "us_per_call": round(us, 1), "us_min": round(mn, 1), "counts": got[3].tolist()}
        dctx.detect_features_raw(jobs, 3000, **params)
        hdr = np.zeros((8, 8), dtype=np.int32)
        n_units = fn(dctx.handle, C.c_void_p(hdr.ctypes.data), 8)
        rec["units"] = [{"candidates": int(h[1]), "accepted": int(h[2]), "corners": int(h[3]), "passes": int(h[4]),
                         "undecided_at_finish": int(h[5])} for h in hdr[:n_units]]
        if not a.no_ref:
            t0 = time.perf_counter()
            want = [G.detect(imgs[cam], e, min_distance=params.get("min_distance", 12.0)) for cam, e in jobs]
            rec["numpy_ref_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            rec["equal_to_ref"] = bool(all(
                got[3][j].tolist() == w[3].tolist() and np.array_equal(got[0][j, :len(w[0])], w[0]) and
                np.array_equal(got[1][j, :len(w[0])].view(np.uint32), w[1].view(np.uint32)) and
                np.array_equal(got[2][j, :len(w[0])].astype(bool), w[2]) for j, w in enumerate(want)))
        out["shapes"][name] = rec
        print(f"{name:11s} {len(jobs)} job(s) {us:9.1f} us/call (min {mn:.1f})  counts {rec['counts']}  units {rec['units']}" +
              (f"  numpy {rec['numpy_ref_ms']:.0f} ms equal={rec['equal_to_ref']}" if not a.no_ref else ""), flush=True)
    ctx.close()
    dctx.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
