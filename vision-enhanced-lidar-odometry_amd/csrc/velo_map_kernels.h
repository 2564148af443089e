// velo_map_kernels.h -- the materialise kernel of the device-resident scan map (velo_map_*, velo_api_map.inl).
// Included by velo_hip.hip (declarations) and by velo_unit_map.hip (VELO_DEF_MAP: the definition); gfx950 only.
//
// The map keeps every scan as it was registered, in its own sensor frame, with a pose.  A load writes the scans of the window into a
// context's target buffer in the frame the caller names: per scan the HOST forms M = ref_inv * pose in double, per point the DEVICE
// computes q_i = ((M_i0 x + M_i1 y) + M_i2 z) + M_i3 in double (the floats widened, the sum left to right, no contraction: the
// library's build flag) and rounds to float once.  No division by a fourth row, no shortcut for an identity: -0.0f comes out +0.0f.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef VELO_DEF_MAP
#define VELO_DEF_MAP 0
#endif

namespace velo {

// One scan of one map of a call.  Read at a workgroup-uniform index (blockIdx.y), so the 120 bytes arrive through the scalar cache.
struct MapUnit {
    const float4* src;       // the scan's block in its map's arena
    float4* dst;             // where its first point goes: the context's target buffer + the points of the scans before it
    int n;                   // points
    int pad;
    double m[12];            // rows 0..2 of M, row-major
};
static_assert(sizeof(MapUnit) == 120, "MapUnit layout");

constexpr int kMapThreads = 256;
constexpr int kMapPerThread = 4;                                       // 16-byte accesses, four per lane: 1,024 points per workgroup
constexpr int kMapTile = kMapThreads * kMapPerThread;

// The pointers come out of the table entry, so the compiler cannot know their address space and would use flat accesses; both are
// device memory (hipMalloc), and the casts say so: global_load / global_store, which leave the LDS counter alone.
typedef float MapF4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) MapF4* MapSrcPtr;
typedef __attribute__((address_space(1))) MapF4* MapDstPtr;

__device__ __forceinline__ MapF4 map_move_point(const MapF4 p, const double* __restrict__ m) {
    const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
    const double qx = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    const double qy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    const double qz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
    MapF4 q;
    q.x = (float)qx; q.y = (float)qy; q.z = (float)qz; q.w = 0.0f;
    return q;
}

// grid (ceil(largest unit / kMapTile), units): a workgroup past the end of its unit returns.  A pure stream, 16 B in and 16 B out
// per point.  A workgroup whose tile lies wholly inside its unit (a workgroup-uniform test: all but the last tile of a scan) issues
// the four 16-byte loads of a lane with no bounds test between them, before the first use (a wave reads 4 x 1 KB contiguous); the
// last tile of a unit takes the guarded path, point by point.
__global__ void __launch_bounds__(kMapThreads)
map_materialise_kernel(const MapUnit* __restrict__ units)
#if VELO_DEF_MAP
{
    const MapUnit& U = units[blockIdx.y];
    const int n = U.n;
    const int tile0 = blockIdx.x * kMapTile;
    if (tile0 >= n) return;
    const MapSrcPtr src = (MapSrcPtr)U.src + tile0;
    const MapDstPtr dst = (MapDstPtr)U.dst + tile0;
    double m[12];
#pragma unroll
    for (int k = 0; k < 12; k++) m[k] = U.m[k];
    const int t = threadIdx.x;
    if (n - tile0 >= kMapTile) {
        MapF4 p[kMapPerThread];
#pragma unroll
        for (int u = 0; u < kMapPerThread; u++) p[u] = src[t + u * kMapThreads];
#pragma unroll
        for (int u = 0; u < kMapPerThread; u++) dst[t + u * kMapThreads] = map_move_point(p[u], m);
    } else {
        const int left = n - tile0;
        for (int j = t; j < left; j += kMapThreads) dst[j] = map_move_point(src[j], m);
    }
}
#else
;
#endif

}  // namespace velo
