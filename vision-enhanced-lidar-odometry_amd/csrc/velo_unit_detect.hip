// velo_unit_detect.hip -- the translation unit that DEFINES the kernels of the VELO_DEF_DETECT family (velo_detect_kernels.h: the
// minimum-eigenvalue corner map, candidate compaction, the parallel minimum-distance selection and the fresh filter): their device code
// is generated here and nowhere else; velo_hip.hip (the host side of the C-ABI) sees declarations and launches through the host stubs
// this unit exports.  No host logic lives here.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/velo_hip.h"

#define VELO_DEF_DETECT 1
#include "velo_detect_kernels.h"
