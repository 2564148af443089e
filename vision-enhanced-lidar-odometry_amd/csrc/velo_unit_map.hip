// velo_unit_map.hip -- the translation unit that DEFINES the kernel of the VELO_DEF_MAP family (velo_map_kernels.h: the materialise
// launch of the device-resident scan map): its device code is generated here and nowhere else; velo_hip.hip (the host side of the
// C-ABI) sees the declaration and launches through the host stub this unit exports.  No host logic lives here.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#define VELO_DEF_MAP 1
#include "velo_map_kernels.h"
