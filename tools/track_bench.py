#!/usr/bin/env python3
"""Feature tracking (velo_set_images + velo_track_features, trackFeatures velo.h:28-116) per call, for the reference's per-frame shape:
    set_images   2 cameras of 1226 x 370 (upload + pyramid + derivatives of every level)
    track        4 jobs x 3,000 points (main.cpp:222-235: for cam, for prev_cam), 21 x 21 window, 5 levels, 30 iterations at most
    contexts     8 contexts one after another, each set_images + track (a host thread driving 8 sequences)
Needs a GPU (it fails without one: there is no CPU path).  Per shape: us per call (median of --iters synchronous calls after --warmup
calls; a host clock around work that ends in a device synchronise), whether the result equals the numpy restatement (tests/lk_ref.py),
the mean iterations per level (the diagnostics build's counters), and the restatement's CPU time as a sanity figure.
Kernel times come from a separate run under `rocprofv3 --kernel-trace --stats` (--no-ref keeps that run short).
Usage: python tools/track_bench.py [--iters 50] [--warmup 5] [--no-ref] [--json out.json]"""
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
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("track_bench: no GPU visible (/dev/kfd missing); this tool measures the device and has no CPU path")
    try:
        import torch  # noqa: F401  (same library load order as bench.py and the tests)
    except Exception:
        pass
    import velo_amd  # noqa: F401
    from velo_amd import api, synth
    import lk_ref as R
    fr = synth.tracking_frames(1226, 370, seed=0)
    pts = [synth.tracking_points(3000, seed=5 + c) for c in range(2)]
    jobs = [(pc, cc, pts[pc]) for cc in range(2) for pc in range(2)]
    out = {"iters": a.iters, "warmup": a.warmup, "shapes": {}}

    ctx = api.Context(0)
    ctx.set_images(fr["prev"])
    ctx.set_images(fr["next"])
    got = ctx.track_features(jobs)

    def upload():
        ctx.set_images(fr["next"])
        ctx.synchronize()
    us, mn = timed(upload, a.iters, a.warmup)
    out["shapes"]["set_images"] = {"cams": 2, "us_per_call": round(us, 1), "us_min": round(mn, 1), "bytes_up": 2 * 1226 * 370}
    print(f"set_images  2 x 1226x370        {us:9.1f} us/call (min {mn:.1f})", flush=True)
    ctx.set_images(fr["prev"])
    ctx.set_images(fr["next"])
    us, mn = timed(lambda: ctx.track_features(jobs), a.iters, a.warmup)
    rec = {"jobs": 4, "points": 12000, "us_per_call": round(us, 1), "us_min": round(mn, 1)}
    if not a.no_ref:
        P = [R.build_pyramid(i) for i in fr["prev"]]
        N = [R.build_pyramid(i) for i in fr["next"]]
        t0 = time.perf_counter()
        want = [R.track_job(P[pc], N[cc], xy) for pc, cc, xy in jobs]
        rec["numpy_ref_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["equal_to_ref"] = bool(all(np.array_equal(got[0][j].view(np.uint32), want[j][0].view(np.uint32)) and
                                       np.array_equal(got[1][j], want[j][1]) and np.array_equal(got[2][j], want[j][2]) for j in range(4)))
    out["shapes"]["track"] = rec
    print(f"track       4 jobs x 3000 points {us:9.1f} us/call (min {mn:.1f})" +
          (f"  numpy {rec['numpy_ref_ms']:.0f} ms equal={rec['equal_to_ref']}" if not a.no_ref else ""), flush=True)
    ctx.close()

    ctxs = [api.Context(0) for _ in range(8)]
    for c in ctxs:
        c.set_images(fr["prev"])

    def frame8():
        for c in ctxs:
            c.set_images(fr["next"])
            c.track_features(jobs)
    us, mn = timed(frame8, max(a.iters // 4, 3), 2)
    out["shapes"]["contexts"] = {"contexts": 8, "us_per_call": round(us, 1), "us_min": round(mn, 1), "us_per_context": round(us / 8, 1)}
    print(f"contexts    8 x (set_images + track) {us:9.1f} us (min {mn:.1f}), {us / 8:.1f} us per context", flush=True)
    for c in ctxs:
        c.close()

    # mean iterations per level: the diagnostics build counts them (velo_diag_track_counters)
    diag = api.load_diagnostics_library()
    fn = diag.velo_diag_track_counters
    fn.restype, fn.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    dc = api.Context(0, lib=diag)
    dc.set_images(fr["prev"])
    dc.set_images(fr["next"])
    dc.track_features(jobs)
    cnt = np.zeros(16, dtype=np.uint64)
    assert fn(dc.handle, C.c_void_p(cnt.ctypes.data), 1) == 0
    dc.close()
    lv = {lev: {"entered": int(cnt[8 + lev]), "iterations": int(cnt[lev]),
                "mean_iterations": round(float(cnt[lev]) / max(int(cnt[8 + lev]), 1), 2)} for lev in range(5)}
    out["iterations_per_level"] = lv
    print("iterations per level (level: mean over the points that entered the loop): " +
          ", ".join(f"{k}: {v['mean_iterations']}" for k, v in sorted(lv.items(), reverse=True)), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
