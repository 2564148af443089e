// velo_unit_landmarks.hip -- the translation unit that DEFINES the kernels of the VELO_DEF_LANDMARKS family (velo_landmark_kernels.h: the
// resident landmark store's append, gather, solve, frame transform and read-back): their device code is generated here and nowhere
// else; velo_hip.hip (the host side of the C-ABI) sees declarations and launches through the host stubs this unit exports.  No host
// logic lives here.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/velo_hip.h"

#define VELO_DEF_LANDMARKS 1
#include "velo_landmark_kernels.h"
