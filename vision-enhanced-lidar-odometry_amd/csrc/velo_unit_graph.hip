// velo_unit_graph.hip -- the translation unit that DEFINES the kernels of the VELO_DEF_GRAPH family (velo_graph_kernels.h: the batch
// optimisation of a drive's pose graph): their device code is generated here and nowhere else; velo_hip.hip (the host side of the
// C-ABI) sees declarations and launches through the host stubs this unit exports.  No host logic lives here.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include "../../include/velo_hip.h"

#define VELO_DEF_GRAPH 1
#include "velo_graph_kernels.h"
