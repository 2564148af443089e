"""CPU test: every kernel header compiles on its own.  A one-line translation unit that includes only that header passes hipcc's
device-side syntax check with the build's flags -- no header relies on what another one happened to include ahead of it."""
import glob
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import velo_amd  # noqa: F401
from velo_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AB_HEADER = "velo_assoc_ab_kernels.h"


def headers():
    found = sorted(os.path.basename(p) for p in glob.glob(os.path.join(build.CSRC, "*_kernels.h")))
    assert AB_HEADER in found and "velo_lm_ag_kernels.h" in found, found      # the glob sees the directory
    return found + ["velo_scan_types.h", "velo_device_math.h", "velo_trust_region.h"]


def test_every_kernel_header_is_self_contained():
    cases = [(h, ()) for h in headers()] + [(AB_HEADER, ("-DVELO_DIAGNOSTICS",))]
    with tempfile.TemporaryDirectory() as td:
        def check(case):
            header, extra = case
            src = os.path.join(td, f"only_{header}_{len(extra)}.hip")
            with open(src, "w") as f:
                f.write(f'#include "{header}"\n')
            r = subprocess.run(["hipcc", *build.HIPCC_FLAGS, *extra, "-I", build.CSRC, "-I", os.path.join(ROOT, "include"),
                                "--cuda-device-only", "-fsyntax-only", src], capture_output=True, text=True)
            return header, extra, r.returncode, r.stderr
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            results = list(pool.map(check, cases))
    bad = [f"{h} {' '.join(extra)}\n{err[-2000:]}" for h, extra, rc, err in results if rc != 0]
    assert not bad, "\n".join(bad)
