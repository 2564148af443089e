#!/usr/bin/env python3
"""The visual front end of n sequences on one GPU, per frame: n single-context calls one after another ("seq") against ONE batch call
("batch") for each of the three stages
    upload   set_images / set_images_batch, 2 cameras per context (timed up to a synchronise of every context: the calls are asynchronous)
    track    track_features / track_features_batch, 4 jobs x 3,000 points per context (main.cpp:222-235)
    detect   detect_features / detect_features_batch, both cameras, 1,500 existing points each, GFTTDetector(3000, 0.001, 12)
Shapes: --n contexts of 1226 x 370 (default 1 2 4 8 16), plus one run with the four mixed sizes 1226 x 370, 1241 x 376, 1242 x 375,
641 x 203 (--no-mixed leaves it out).  Needs a GPU (it fails without one: there is no CPU path).  Per stage and shape: us (median and
minimum of --iters calls after --warmup; a host clock around work that ends in a device synchronise), and whether the batch call's
outputs equal the single calls' byte for byte.
    --lib PATH       time ANOTHER build of the library (an A/B build of an earlier commit: it may lack the batch entries; only "seq"
                     is measured then) -- the baseline a change is held against, measured in the same visit
    --modes seq      "seq", "batch" or both (default); --stages upload track detect
Kernel times and launches per call come from a run of their own under `rocprofv3 --kernel-trace --stats` with --iters small and one
--n / one mode, e.g.  rocprofv3 --kernel-trace --stats -d out -- python tools/frontend_batch_bench.py --n 8 --modes batch --no-mixed --iters 20
Usage: python tools/frontend_batch_bench.py [--n 1 2 4 8 16] [--iters 200] [--warmup 10] [--lib PATH] [--json out.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

MIXED = [(1226, 370), (1241, 376), (1242, 375), (641, 203)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(statistics.median(ts) * 1e6, 1), round(min(ts) * 1e6, 1)


def same_bytes(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bytes(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 2, 4, 8, 16])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--modes", nargs="+", default=["seq", "batch"], choices=["seq", "batch"])
    ap.add_argument("--stages", nargs="+", default=["upload", "track", "detect"], choices=["upload", "track", "detect"])
    ap.add_argument("--no-mixed", action="store_true")
    ap.add_argument("--lib", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not os.path.exists("/dev/kfd"):
        sys.exit("frontend_batch_bench: no GPU visible (/dev/kfd missing); this tool measures the device and has no CPU path")
    try:
        import torch  # noqa: F401  (same library load order as bench.py and the tests)
    except Exception:
        pass
    import velo_amd  # noqa: F401
    from velo_amd import api, synth
    lib = None
    if a.lib:                                                   # another build: type what it exports, it may predate some entries
        lib = C.CDLL(a.lib, mode=C.RTLD_GLOBAL)
        for name, (res, args) in api.SIGNATURES.items():
            if hasattr(lib, name):
                getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    has_batch = lib is None or hasattr(lib, "velo_set_images_batch")
    modes = [m for m in a.modes if m == "seq" or has_batch]
    out = {"iters": a.iters, "warmup": a.warmup, "lib": a.lib or "product", "modes": modes, "shapes": {}}
    shapes = [(f"{n} x 1226x370", [(1226, 370)] * n) for n in a.n]
    if not a.no_mixed:
        shapes.append(("mixed " + " ".join(f"{w}x{h}" for w, h in MIXED), MIXED))
    frames = {}
    for name, sizes in shapes:
        n = len(sizes)
        for i, (w, h) in enumerate(sizes):
            if (w, h, i) not in frames:
                frames[(w, h, i)] = synth.tracking_frames(w, h, seed=i)
        fr = [frames[(w, h, i)] for i, (w, h) in enumerate(sizes)]
        ctxs = [api.Context(0, lib=lib) for _ in range(n)]
        for c, f in zip(ctxs, fr):
            c.set_images(f["prev"])
            c.set_images(f["next"])
        nxt = [f["next"] for f in fr]
        tjobs, djobs = [], []
        for i, (w, h) in enumerate(sizes):
            pts = [synth.tracking_points(3000, w, h, seed=5 + 2 * i + c) for c in range(2)]
            tjobs += [(i, pc, cc, pts[pc]) for cc in range(2) for pc in range(2)]
            djobs += [(i, cam, synth.tracking_points(1500, w, h, seed=50 + 2 * i + cam)) for cam in range(2)]
        t_per = [[j[1:] for j in tjobs if j[0] == i] for i in range(n)]
        d_per = [[j[1:] for j in djobs if j[0] == i] for i in range(n)]

        def sync_all():
            for c in ctxs:
                c.synchronize()

        def upload_seq():
            for c, im in zip(ctxs, nxt):
                c.set_images(im)
            sync_all()

        def upload_batch():
            api.set_images_batch(ctxs, nxt)
            sync_all()

        def track_seq():
            return [c.track_features(j) for c, j in zip(ctxs, t_per)]

        def track_batch():
            return api.track_features_batch(ctxs, tjobs)

        def detect_seq():
            return [c.detect_features_raw(j, 3000) for c, j in zip(ctxs, d_per)]

        def detect_batch():
            return api.detect_features_batch_raw(ctxs, djobs, 3000)

        fns = {"upload": (upload_seq, upload_batch), "track": (track_seq, track_batch), "detect": (detect_seq, detect_batch)}
        rec = {"contexts": n}
        for stage in a.stages:
            for k, mode in enumerate(("seq", "batch")):
                if mode in modes:
                    med, mn = timed(fns[stage][k], a.iters, a.warmup)
                    rec[f"{stage}_{mode}_us"], rec[f"{stage}_{mode}_us_min"] = med, mn
        if "batch" in modes and "seq" in modes:                 # after the timed loops: the slots hold `next` twice, for both alike
            if "track" in a.stages:
                s, b = track_seq(), track_batch()
                rec["track_equal"] = all(same_bytes([s[i][r][k] for i in range(n) for k in range(4)], b[r]) for r in range(3))
            if "detect" in a.stages:
                s, b = detect_seq(), detect_batch()
                rec["detect_equal"] = all(same_bytes(np.concatenate([s[i][r] for i in range(n)]), b[r]) for r in range(4))
        out["shapes"][name] = rec
        line = f"{name:46s}"
        for stage in a.stages:
            for mode in modes:
                line += f"  {stage}/{mode} {rec[f'{stage}_{mode}_us']:9.1f} (min {rec[f'{stage}_{mode}_us_min']:.1f})"
        line += "".join(f"  {k}={rec[k]}" for k in ("track_equal", "detect_equal") if k in rec)
        print(line, flush=True)
        for c in ctxs:
            c.close()
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
