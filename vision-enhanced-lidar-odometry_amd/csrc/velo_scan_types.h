// velo_scan_types.h -- constants and device data layouts that more than one kernel family reads (gfx950 / CDNA4 only): the search grid,
// the pose scalars of an association round, the hand-over records of chain mode and of the target-sharded mode, the visual match record, the workgroup scan.  No kernel lives here.
// velo_load_kernels.h and velo_kernels.h (the scan-matching core) build on it; the bundle adjustment, pose graph, landmark and frame headers include it
// instead of the core's kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "velo_device_math.h"
#include "velo_trust_region.h"   // LMParams

namespace velo {

constexpr int kWave = 64;
constexpr int kNumAcc = 28;           // 21 upper-triangular JtJ + 6 Jtr + cost
constexpr int kEvalThreads = 256;
constexpr int kMaxEvalBlocks = 512;
constexpr int kAssocThreads = 256;

// ---- uniform grid over the target cloud (one per distinct gate radius) ------------------------------------
struct GridDesc {
    float ox, oy, oz;       // origin = bbox min
    float inv_h;            // 1 / cell size (one fine grid, cell ~ 1.01 x the smallest gate radius, serves every gate)
    int nx, ny, nz;
    int ncells;
};

// Cell-sorted copy of the target: float4 {x, y, z, bits(global ring-major target index)} + the point's ring, so that a
// workgroup can stage whole cell runs into LDS with one coalesced 16-byte load per candidate.  kGridPad sentinel
// entries (x = +inf) follow the last real point.
constexpr int kGridPad = 16;
struct GridView {
    GridDesc d;
    const int* __restrict__ cell_start;      // dense: [ncells + 1] start of every cell; compressed: start of every OCCUPIED cell, [n_occupied + 1]
    const float4* __restrict__ sorted;       // [n_finite + kGridPad]
    const int* __restrict__ sring;           // ring of sorted[j]
    // Compressed table (large grids: an accumulated map's millions of cells, of which a few per cent hold points): per row (y, z) of
    // the grid `wpr` 64-bit words, bit x & 63 of word x >> 6 = "cell x of this row is occupied", and the number of occupied cells before
    // each word.  start(row, x) = cell_start[wprefix[w] + popcount(wmask[w] below bit x)] -- 0.19 bytes per cell instead of 4, so the
    // table of the 2M-point map (11 M cells) is 2 MB and stays in every XCD's L2, at the price of one dependent load per look-up.
    const unsigned long long* __restrict__ wmask;   // null: dense table
    const int* __restrict__ wprefix;
    int wpr;                                  // words per row = ceil(nx / 64)
};
// first sorted point of cell x (0..nx: nx = one past the row's last cell) of grid row `row` = z * ny + y
__device__ __forceinline__ int grid_start(const GridView& G, int row, int x) {
    if (G.wmask == nullptr) return G.cell_start[row * G.d.nx + x];
    const int w = row * G.wpr + (x >> 6);
    const unsigned long long m = G.wmask[w];
    const int k = G.wprefix[w] + __popcll(m & ((1ull << (x & 63)) - 1ull));
    return G.cell_start[k];
}

// ---- pose scalars of one association round, computed on the HOST in double with the same libm the CPU
// restatement uses, so that the float coordinates of the transformed queries are bit-identical (row A1) -----
struct PoseScalars {
    double w[3];     // omega
    double t[3];
    double c, s;     // cos / sin(theta)
    double u[3];     // omega / theta
    double omc;      // 1 - cos(theta)
    int small;       // theta^2 <= DBL_EPSILON -> first-order branch
};

// the same for host and device: with the pinned sin / cos (velo_device_math.h) and correctly rounded sqrt and division the device
// computes a round's pose scalars with the bits the host (and the oracle) gets, so a frame_to_frame can run as ONE chain of launches
__host__ __device__ inline void pose_scalars_compute(const double x[6], PoseScalars* S) {
    for (int k = 0; k < 3; k++) { S->w[k] = x[k]; S->t[k] = x[3 + k]; S->u[k] = 0.0; }
    S->c = 0.0; S->s = 0.0; S->omc = 0.0;
    const double theta2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (theta2 > 2.220446049250313e-16) {
        const double theta = sqrt(theta2);
        velo_sincos(theta, &S->s, &S->c);
        const double ti = 1.0 / theta;
        S->u[0] = x[0] * ti; S->u[1] = x[1] * ti; S->u[2] = x[2] * ti;
        S->omc = 1.0 - S->c;
        S->small = 0;
    } else {
        S->small = 1;
    }
}
// Device-driven rounds ("chain mode"): the LM step that finishes a solve leaves the pose scalars of its result here, and the next
// round's association kernel reads them -- no host round trip between a solve and the next association.  ready = 0 while a solve
// is running: an association kernel that finds it so was enqueued behind a solve that needed more launches than the host had
// predicted; it raises the chain's failure flag and everything behind it returns at once (the host then repeats the call).
struct PoseRecord {
    PoseScalars P;
    int ready;
    int pad;
};
// what the host wants to know about a finished solve (velo_solve_summary), left by the step that finished it
struct SolveLog {
    double x[6];
    double initial_cost, final_cost;
    int termination, iter, evals, n_valid;
};
// Target-sharded mode (BASELINE config 5): what one rank knows about a query after searching ITS rings.
// Rings are disjoint across ranks, so the global winners are: best1 = min key1 over ranks (rank w*), best2 = the smaller
// of { min key1 over the other ranks, key2 of rank w* }.  The record carries the points the plane needs, so the owner of
// the query can finish without touching any other rank's cloud.  Same layout as velo_partial in include/velo_hip.h.
struct PartialRec {
    unsigned long long key1, key2;     // (d^2 bits << 32 | global index); >= key_inf when absent
    int ring1, ring2;                  // global ring ids, -1 when absent
    int idx1, idx_k, idx2, pad;        // np_i, np_k (in ring1), np_j (in ring2)
    float v0[3], v2[3], v1[3];         // best point, its chosen ring neighbour, second-best point
    float pad2;
};

__device__ __forceinline__ int cell_coord(float p, float o, float inv_h, int n) {
    float f = (p - o) * inv_h;
    f = fminf(fmaxf(f, -2.0f), (float)(n + 1));
    return (int)floorf(f);
}

// One record per visual match, three block slots: slot 0 = 3D3D or 2D2D, slot 1 = 3D2D, slot 2 = 2D3D (velo.h order).  The solver reads
// them (velo_kernels.h), the match assembly from resident frames writes them (velo_frame_kernels.h).
struct VisualMatch {      // device copy of velo_match, floats kept as floats and widened at use (costfunctions.h ctors)
    float p3_1[3], p3_2[3], p2_1[2], p2_2[2], t_cam[3];
    int cam, point1, point2;
    unsigned char d1, d2, pad[2];
};

// ---- workgroup scan: the load family's index build, the depth rows and the frame kernels compact with it ----------------------------
constexpr int kScanThreads = 256;
constexpr int kScanItems = 8;                      // per thread
constexpr int kScanTile = kScanThreads * kScanItems;

__device__ __forceinline__ int block_exclusive_scan(int v, int* total) {
    __shared__ int wave_sums[kScanThreads / kWave];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int t = __shfl_up(inc, off); if (lane >= off) inc += t; }
    if (lane == 63) wave_sums[wid] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kScanThreads / kWave; w++) { const int s = wave_sums[w]; if (w < wid) base += s; tot += s; }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// Work item of the pipelined A/B association (velo_assoc_ab_kernels.h).  Shared because the host's context type declares a buffer of
// them in both builds (reserved only when the diagnostics build runs that variant: the product never allocates it).
struct AssocItem {            // 32 bytes
    int group;                // 64-query group
    unsigned mask_lo, mask_hi;
    int bx, by, bz;           // cell bounding box of the members: lo | hi << 16
    int pad0, pad1;
};

}  // namespace velo
