"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol include/velo_hip.h declares,
agrees with the header on struct layout, and FAILS LOUDLY without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_lib as ol
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "velo_hip.h")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()                       # hipcc cross-compiles gfx950 without a GPU
    return api.load_library()


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(velo_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(lib):
    names = declared_functions()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/velo_hip.h but not exported"
    assert set(names) == set(api.SIGNATURES), set(names) ^ set(api.SIGNATURES)


def test_struct_layouts_match_the_header():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "velo_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu\n", sizeof(velo_params), sizeof(velo_match), sizeof(velo_good_match), sizeof(velo_corr),
         sizeof(velo_solve_summary), sizeof(velo_summary));
  printf("%zu %zu %zu %zu\n", offsetof(velo_params, weight_3D2D), offsetof(velo_match, cam), offsetof(velo_corr, p), offsetof(velo_summary, solves));
  printf("%zu %zu %zu %zu %zu\n", sizeof(velo_tri_obs), sizeof(velo_tri_result), sizeof(velo_partial), sizeof(velo_functor), offsetof(velo_functor, c));
  printf("%zu %zu %zu\n", sizeof(velo_residual_stats), offsetof(velo_summary, residual_stats), offsetof(velo_residual_stats, cost));
  return 0; }
'''
    with tempfile.TemporaryDirectory() as td:
        cfile = os.path.join(td, "probe.c")
        open(cfile, "w").write(src)
        exe = os.path.join(td, "probe")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)  # the header is plain C
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    sizes = [int(v) for v in out]
    assert sizes[:6] == [C.sizeof(api.VeloParams), api.MATCH_DTYPE.itemsize, api.GOOD_DTYPE.itemsize, api.CORR_DTYPE.itemsize,
                         C.sizeof(api.VeloSolveSummary), C.sizeof(api.VeloSummary)]
    assert sizes[6] == api.VeloParams.weight_3D2D.offset
    assert sizes[7] == api.MATCH_DTYPE.fields["cam"][1]
    assert sizes[8] == api.CORR_DTYPE.fields["p"][1]
    assert sizes[9] == api.VeloSummary.solves.offset
    assert sizes[10:15] == [api.TRI_OBS_DTYPE.itemsize, api.TRI_RESULT_DTYPE.itemsize, api.PARTIAL_DTYPE.itemsize,
                            api.FUNCTOR_DTYPE.itemsize, api.FUNCTOR_DTYPE.fields["c"][1]]
    assert sizes[15:18] == [C.sizeof(api.VeloResidualStats), api.VeloSummary.residual_stats.offset, api.VeloResidualStats.cost.offset]


def test_default_params_are_the_reference_constants(lib):
    p = api.VeloParams()
    assert lib.velo_default_params(C.byref(p)) == 0
    # kitti.h:8-10,20-26,30-32
    assert (p.icp_skip, p.f2f_iterations, p.icp_iterations) == (200, 2, 3)
    assert (p.weight_3D2D, p.weight_2D2D, p.weight_3DPD) == (10, 500, 1)
    assert (p.loss_thresh_3D2D, p.loss_thresh_2D2D, p.loss_thresh_3DPD, p.loss_thresh_3D3D) == (0.01, 0.00002, 0.1, 0.04)
    assert (p.outlier_reject, p.correspondence_thresh_icp, p.icp_norm_condition) == (5.0, 0.5, 1e-5)
    assert (p.enable_icp, p.enable_2d2d, p.enable_3d2d) == (1, 1, 1)
    q, o = api.default_params(), ol.default_params()
    for name, _ in api.VeloParams._fields_:
        assert getattr(p, name) == getattr(q, name) == getattr(o, name), name


def test_pose_helpers_match_oracle(lib):
    rng = np.random.default_rng(5)
    for _ in range(20):
        x = np.concatenate([rng.normal(size=3) * 0.7, rng.normal(size=3)])
        T = api.pose_vec_to_mat(x)
        np.testing.assert_allclose(T, ol.pose_vec_to_mat(x), atol=1e-15)
        np.testing.assert_allclose(api.pose_mat_to_vec(T), x, atol=1e-13)
    np.testing.assert_array_equal(api.pose_vec_to_mat(np.zeros(6)), np.eye(4))


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this check is for boxes without a GPU")
def test_no_gpu_means_loud_failure_not_fallback(lib):
    h = C.c_void_p()
    st = lib.velo_create(C.byref(h), 0)
    assert st == -5 and not h.value                      # VELO_ERR_NODEVICE
    assert b"no CPU fallback" in lib.velo_last_error()
    with pytest.raises(api.VeloError):
        api.Context(0)


def test_argument_validation_without_gpu(lib):
    assert lib.velo_default_params(None) == -1
    assert lib.velo_destroy(None) == 0
    assert lib.velo_pose_vec_to_mat(None, None) == -1
    assert lib.velo_set_params(None, None) == -1
    assert lib.velo_version().startswith(b"velo_hip")
    # batch entry point: a context listed twice (it would race with itself) or a null entry is refused before anything is touched
    x = (C.c_double * 12)()
    fake = C.c_void_p(0x1000)
    arr = (C.c_void_p * 2)(fake, fake)
    assert lib.velo_frame_to_frame_batch(arr, 2, x, None, None) == -1 and b"same context" in lib.velo_last_error()
    arr = (C.c_void_p * 2)(fake, None)
    assert lib.velo_frame_to_frame_batch(arr, 2, x, None, None) == -1 and b"null" in lib.velo_last_error()
    assert lib.velo_frame_to_frame_batch(arr, 0, x, None, None) == 0
    assert lib.velo_cache_create(None, 0, 50) == -1 and lib.velo_cache_destroy(None) == 0 and lib.velo_cache_contains(None, 3) == 0
    assert lib.velo_evaluate_functors(None, None, 0, None, None, None) == -1


def test_product_never_touches_the_oracle():
    """Nothing under the package directory may import, link or execute anything under oracle/."""
    pkg = os.path.join(ROOT, "vision-enhanced-lidar-odometry_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".hpp", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle_lib" not in text and "libvelo_oracle" not in text and "velo_oracle" not in text, (dirpath, f)
    out = subprocess.run(["ldd", build.LIB], capture_output=True, text=True).stdout
    assert "oracle" not in out


PRODUCT_KNOBS = {"VELO_CHAIN", "VELO_CHAIN_MARGIN", "VELO_BATCH_GROUPS", "VELO_BATCH_LOCKSTEP", "VELO_SPIN"}


def test_product_library_reads_only_the_documented_environment_knobs():
    """The product library's environment surface is the five result-preserving knobs include/velo_hip.h documents; every A/B switch
    (kernel variants, grid shapes, diagnostics) lives in the -DVELO_DIAGNOSTICS build only -- checked on the binaries themselves."""
    import re
    def names(path):
        data = open(path, "rb").read()
        return {m.decode() for m in re.findall(rb"(?<![A-Z_0-9])VELO_[A-Z_0-9]+(?=\x00)", data)}
    assert names(build.LIB) == PRODUCT_KNOBS, names(build.LIB)
    diag = build.build_hip(diagnostics=True)
    extra = names(diag) - PRODUCT_KNOBS
    assert {"VELO_ASSOC_VARIANT", "VELO_DEBUG_SKIP", "VELO_WARM_START", "VELO_DENSE_REF", "VELO_LM_FUSED"} <= extra
    header = open(os.path.join(ROOT, "include", "velo_hip.h")).read()
    for k in PRODUCT_KNOBS:
        assert k in header, k                              # documented where the boundary is declared


AB_KERNELS = (b"19assoc_search_kernel", b"22assoc_search_v3_kernel", b"17assoc_lane_kernel", b"23assoc_lane_batch_kernel",
              b"20assoc_prepare_kernel", b"20assoc_cluster_kernel")


def test_product_library_holds_no_ab_association_kernel():
    """The A/B association kernels (velo_assoc_ab_kernels.h) are launched by the -DVELO_DIAGNOSTICS build only, so only that build
    holds them -- checked on the binaries themselves, by the length-prefixed part of their mangled names."""
    build.build_hip()
    product = open(build.LIB, "rb").read()
    found = [k.decode() for k in AB_KERNELS if k in product]
    assert not found, found
    diag = open(build.build_hip(diagnostics=True), "rb").read()
    missing = [k.decode() for k in AB_KERNELS if k not in diag]
    assert not missing, missing
