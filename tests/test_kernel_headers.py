"""CPU test: every kernel header compiles on its own.  A one-line translation unit that includes only that header passes hipcc's
device-side syntax check with the build's flags -- no header relies on what another one happened to include ahead of it."""
import glob
import os
import re
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
    assert "velo_load_kernels.h" in found, found
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


def test_load_family_has_left_the_shared_header():
    """The load family lives in velo_load_kernels.h alone: only that header and the widened rows the load unit also defines gate code by
    VELO_DEF_LOAD or name the family's instantiation list, the load unit reads no other scan-matching header, PartialRec has one
    definition and no forward declaration, and each family flag of the core is set to 1 by exactly one unit."""
    texts = {}
    for pattern in ("*.h", "*.hip", "*.inl"):
        for p in glob.glob(os.path.join(build.CSRC, pattern)):
            with open(p) as f:
                texts[os.path.basename(p)] = f.read()
    assert len(texts) > 40, sorted(texts)
    gated = sorted(n for n, t in texts.items() if n.endswith(".h") and re.search(r"^[ \t]*#[ \t]*if.*VELO_DEF_LOAD", t, re.M))
    assert gated == ["velo_depth_kernels.h", "velo_load_kernels.h", "velo_tri_kernels.h"], gated
    assert [n for n, t in texts.items() if "VELO_INST_LOAD" in t] == ["velo_load_kernels.h"]
    included = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"(velo_[a-z_]+\.h)"', texts["velo_unit_load.hip"], re.M)
    assert included == ["velo_load_kernels.h", "velo_depth_kernels.h", "velo_tri_kernels.h"], included
    assert re.findall(r'^[ \t]*#[ \t]*include[ \t]+"(velo_[a-z_]+\.h)"', texts["velo_load_kernels.h"], re.M) == ["velo_scan_types.h"]
    assert [n for n, t in texts.items() if re.search(r"^struct PartialRec \{", t, re.M)] == ["velo_scan_types.h"]
    assert not [n for n, t in texts.items() if "struct PartialRec;" in t]
    for flag in ("VELO_DEF_LOAD", "VELO_DEF_ASSOC", "VELO_DEF_LMA", "VELO_DEF_LMB"):
        setters = sorted(n for n, t in texts.items() if re.search(rf"^[ \t]*#[ \t]*define[ \t]+{flag}[ \t]+1\b", t, re.M))
        assert len(setters) == 1 and setters[0].endswith(".hip"), (flag, setters)
