// velo_unit_frames.hip -- the translation unit that DEFINES the kernels of the VELO_DEF_FRAMES family (velo_frame_kernels.h: the
// match assembly from resident keypoint frames -- slot fill, chunk counts, record emit, slot clear; the prune; the fr_depth_* kernels of
// a frame put with its depth, which inline the device functions of velo_depth_kernels.h): their device code is generated
// here and nowhere else; velo_hip.hip (the host side of the C-ABI) sees declarations and launches through the host stubs this unit
// exports.  No host logic lives here.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/velo_hip.h"

#define VELO_DEF_FRAMES 1
#include "velo_frame_kernels.h"
