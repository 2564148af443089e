// velo_unit_assoc.hip -- the translation unit that DEFINES the kernels of the VELO_DEF_ASSOC family (velo_hip.hip, "translation units"): their
// device code is generated here and nowhere else; velo_hip.hip (the host side of the C-ABI) and the other units see declarations and launch
// through the host stubs this unit exports.  No host logic lives here.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/velo_hip.h"

#define VELO_DEF_ASSOC 1
#include "velo_kernels.h"
#ifdef VELO_DIAGNOSTICS
#include "velo_assoc_ab_kernels.h"   // the A/B kernels exist in the diagnostics build only
#endif
