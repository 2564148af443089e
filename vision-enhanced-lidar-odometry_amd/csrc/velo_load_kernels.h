// velo_load_kernels.h -- how a scan enters a context and becomes a search index (gfx950 / CDNA4 only): point packing, the query list in
// patch order, scan ingestion (ring segmentation), the bounding box, the uniform grid (count / look-back scan / scatter, cell >= gate
// radius) and the advance_* loaders that do the same for every context of a lock-step group in one launch.
// Defined in velo_unit_load.hip (VELO_DEF_LOAD); every other unit sees declarations (velo_hip.hip, "translation units").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "velo_scan_types.h"   // constants, grid, pose scalars, hand-over records; velo_device_math.h, velo_trust_region.h (LMParams)

#ifndef VELO_DEF_LOAD
#define VELO_DEF_LOAD 0
#endif

namespace velo {

// ---- point packing: (stride-addressed xyz) -> float4 ---------------------------------------------------------
// records from page-locked host memory into a device buffer, as a launch: the runtime's copy of a few tens of KB (its DMA path) was seen to
// block the submitting thread for 6-14 ms once in a hundred steps with four busy queues; a launch never does
__global__ void __launch_bounds__(256) upload_words_kernel(const int* __restrict__ src, int* __restrict__ dst, int n_words)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) dst[i] = __builtin_nontemporal_load(src + i);
}
#else
;
#endif
__global__ void pack_points_kernel(const char* __restrict__ src, int64_t stride, int n, float4* __restrict__ dst)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = (const float*)(src + (int64_t)i * stride);
    dst[i] = make_float4(p[0], p[1], p[2], 0.0f);
}
#else
;
#endif

// ring id per point (binary search in ring_offsets) -- the target's gidx -> ring map
// (a context may hold only a block of whole rings of the target -- target-sharded mode -- so ring ids and point
//  indices that leave the kernels are GLOBAL: local ring + first_ring, local index + first_point)
// (bbox_init: the six keys bbox_kernel folds into -- min keys all ones, max keys zero -- are initialised here, one launch ahead of it,
//  instead of by a copy operation of their own)
__global__ void ring_of_kernel(const int* __restrict__ off, int n_rings, int n, int first_ring, int* __restrict__ ring_of, unsigned* __restrict__ bbox_init)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (bbox_init && i < 6) bbox_init[i] = i < 3 ? 0xffffffffu : 0u;
    if (i >= n) return;
    int lo = 0, hi = n_rings;   // find r with off[r] <= i < off[r+1]
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
    ring_of[i] = lo + first_ring;
}
#else
;
#endif

// Ring-major copy of the target with one wrap-around sentinel on either side of every ring:
//     ring r (n_r points at [off[r], off[r+1])) -> pad[off[r] + 2 r] = its LAST point, then its points, then its FIRST point,
// so the cyclic ring neighbours (velo.h:852-854) of point i of local ring r are pad[i + 2 r] and pad[i + 2 r + 2], whatever i:
// the finish of the association reads three adjacent records and needs neither the ring bounds nor a second trip for the wrap.
__global__ void pad_rings_kernel(const float4* __restrict__ tgt, const int* __restrict__ off, const int* __restrict__ ring_of, int n, int first_ring,
                                 float4* __restrict__ pad)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = ring_of[i] - first_ring, base = off[r], end = off[r + 1];
    const float4 p = tgt[i];
    pad[i + 2 * r + 1] = p;
    if (i == base) pad[end + 2 * r + 1] = p;          // trailing sentinel = first point
    if (i == end - 1) pad[base + 2 * r] = p;          // leading sentinel = last point
}
#else
;
#endif

// compact query points: qpts[i] = src[q_src[i]] (icp_skip > 1; with icp_skip == 1 the source cloud itself is the list)
__global__ void gather_queries_kernel(const float4* __restrict__ src, const int* __restrict__ q_src, int nq, float4* __restrict__ qpts)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nq) qpts[i] = src[q_src[i]];
}
#else
;
#endif

// ---- patch order of the queries ---------------------------------------------------------------------------------------------------
// The tube kernel gives 64 consecutive queries to a workgroup.  In ring order that is a 2 m long line of one ring (a tube of ~125
// cells); the same 64 queries taken as 8 neighbouring rings x 8 consecutive points are a patch of ~0.5 m x 0.25 m (~60 cells):
// fewer rows, fewer staged candidates, tighter bounds.  So the query LIST is laid out in patch order: bands of kPatchRings source
// rings, each ring of a band cut into the same number M of segments (M = ceil(longest ring of the band / kPatchLen)); the list runs
// band by band, segment by segment, ring by ring, point by point.  Everything indexed by query (seeds, table, LM rows) follows the
// list; the results per query are what they were, and the calls that hand tables out restore ring order (patch_position is the map,
// the same integer arithmetic on host and device).  Closed form, no sort: segment j of a ring with n queries starts at ceil(j n / M).
constexpr int kPatchRingsDefault = 8, kPatchLenDefault = 8;      // (4 x 16, 16 x 4, 2 x 32, 8 x 4, 4 x 8 measured within 3 % or worse)
__host__ __device__ inline int patch_first(int j, int n, int M) { return (int)(((long long)j * n + M - 1) / M); }
__host__ __device__ inline int patch_position(const int* q_off, int n_rings, int r, int k, int kPatchRings = 8, int kPatchLen = 8) {
    const int r0 = (r / kPatchRings) * kPatchRings, r1 = (r0 + kPatchRings < n_rings) ? r0 + kPatchRings : n_rings;
    int nmax = 0;
    for (int rr = r0; rr < r1; rr++) { const int nn = q_off[rr + 1] - q_off[rr]; nmax = nn > nmax ? nn : nmax; }
    const int M = (nmax + kPatchLen - 1) / kPatchLen > 1 ? (nmax + kPatchLen - 1) / kPatchLen : 1;
    const int n = q_off[r + 1] - q_off[r];
    const int j = (int)((long long)k * M / n);                        // segment of this query: first(j) <= k < first(j + 1)
    int pos = q_off[r0];                                               // the earlier bands
    for (int rr = r0; rr < r1; rr++) {
        const int nn = q_off[rr + 1] - q_off[rr];
        const int f = patch_first(j, nn, M);
        pos += f;                                                      // the earlier segments of every ring of the band
        if (rr < r) pos += patch_first(j + 1, nn, M) - f;              // this segment of the earlier rings
    }
    return pos + (k - patch_first(j, n, M));
}
// query list: position -> global source index.  Ring r contributes ceil(n_r / skip) queries (velo.h:806-807); patch != 0: the list is
// in patch order, else in the reference's order (ring by ring).
__global__ void query_list_kernel(const int* __restrict__ src_off, const int* __restrict__ q_off, int n_rings,
                                  int skip, int nq, int patch, int patch_rings, int patch_len, int* __restrict__ q_src)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    int lo = 0, hi = n_rings;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (q_off[mid] <= i) lo = mid; else hi = mid; }
    const int k = i - q_off[lo];
    q_src[patch ? patch_position(q_off, n_rings, lo, k, patch_rings, patch_len) : i] = src_off[lo] + k * skip;
}
#else
;
#endif

// ---- scan ingestion on the device: KITTI records -> camera-0-frame rings (kitti.h:121-185), "next" row 1 of SURVEY 8(f) ----
// 1. ring_break_kernel: flag[i] = i > 0 && x_i > 0 && (y_i > 0) != (y_{i-1} > 0)            (kitti.h:164-168, velodyne frame)
// 2. exclusive scan of the flags (scan_tiles/sums/add above) -> ring id per point, ring count
// 3. ring_offsets_kernel: off[ring] = first point of that ring (the flagged points), off[n_rings] = n
// 4. ring_reorder_kernel: camera-frame copy  q = velo_to_cam * p  in float, stored at  new[i] = old[n-1-((i + n/2) % n)]  (kitti.h:178-183)
__global__ void ring_break_kernel(const char* __restrict__ rec, int64_t stride, int n, int* __restrict__ flag)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = (const float*)(rec + (int64_t)i * stride);
    int f = 0;
    if (i > 0) {
        const float* q = (const float*)(rec + (int64_t)(i - 1) * stride);
        f = (p[0] > 0.f && ((p[1] > 0.f) != (q[1] > 0.f))) ? 1 : 0;
    }
    flag[i] = f;
}
#else
;
#endif
// ring_id[i] = (exclusive scan of flag)[i] + flag[i]; the flagged points start rings 1.., point 0 starts ring 0
__global__ void ring_offsets_kernel(const int* __restrict__ excl, const int* __restrict__ flag, int n, int* __restrict__ ring_id, int* __restrict__ off,
                                    int* __restrict__ n_rings_out)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = excl[i] + flag[i];
    ring_id[i] = r;
    if (i == 0 || flag[i]) off[r] = i;
    if (i == n - 1) { off[r + 1] = n; *n_rings_out = r + 1; }
}
#else
;
#endif
struct Mat34f { float m[12]; };   // rows of velo_to_cam (kitti.h:100-107)
__global__ void ring_reorder_kernel(const char* __restrict__ rec, int64_t stride, int n, const int* __restrict__ ring_id, const int* __restrict__ off,
                                    Mat34f M, float4* __restrict__ dst)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* p = (const float*)(rec + (int64_t)i * stride);
    const float x = p[0], y = p[1], z = p[2];
    // pcl::transformPointCloud<float> [3P]: linear part column by column, then the translation, all in float
    const float cx = ((M.m[0] * x + M.m[1] * y) + M.m[2] * z) + M.m[3];
    const float cy = ((M.m[4] * x + M.m[5] * y) + M.m[6] * z) + M.m[7];
    const float cz = ((M.m[8] * x + M.m[9] * y) + M.m[10] * z) + M.m[11];
    const int r = ring_id[i], base = off[r], m = off[r + 1] - base, j = i - base;
    // new[i'] = old[m-1-((i' + m/2) % m)]  <=>  i' = (m-1-j - m/2) mod m
    int ip = (m - 1 - j - m / 2) % m;
    if (ip < 0) ip += m;
    dst[base + ip] = make_float4(cx, cy, cz, 0.f);
}
#else
;
#endif

// ---- bounding box of the finite points: per-block min/max then atomics on order-preserving integer keys ----
__device__ __forceinline__ unsigned f2key(float f) { unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__host__ __device__ __forceinline__ float key2f(unsigned k) {
    unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(u);
#else
    float f; __builtin_memcpy(&f, &u, 4); return f;
#endif
}
__global__ void __launch_bounds__(256)
bbox_kernel(const float4* __restrict__ pts, int n, unsigned* __restrict__ mnmx /* [6]: min xyz, max xyz keys */)
#if VELO_DEF_LOAD
{
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 p = pts[i];
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
            mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off));
        }
    }
    __shared__ float red[4][6];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { for (int k = 0; k < 3; k++) { red[wid][k] = mn[k]; red[wid][3 + k] = mx[k]; } }
    __syncthreads();
    if (threadIdx.x < 6) {     // one atomic per block and component (same-address atomics serialise)
        const int k = threadIdx.x;
        float v = red[0][k];
        for (int w = 1; w < 4; w++) v = (k < 3) ? fminf(v, red[w][k]) : fmaxf(v, red[w][k]);
        if (k < 3) atomicMin(&mnmx[k], f2key(v)); else atomicMax(&mnmx[k], f2key(v));
    }
}
#else
;
#endif

// ---- a scan enters a context in ONE launch per side -----------------------------------------------------------------------------------
// With several registrations in flight a queue operation costs 5-10 us of hand-over whatever it does, and loading a pair used to take
// sixteen of them (pack, ring ids, padded rings, bounding box, two clears, ... each a launch or a copy of its own) against ~30 for the
// registration itself.  target_ingest_kernel is pack_points + ring_of + pad_rings + bbox (and clears the scan's status words);
// source_ingest_kernel is pack_points + query_list + gather_queries (the query blocks read the caller's records themselves, so they
// do not wait for the packed copy).  Same arithmetic, same tables as the separate kernels, which the other entries keep using.
constexpr int kIngestPerThread = 4;                                    // points per thread: 1,024 per workgroup, 6 bounding-box atomics per workgroup at most
// IN-PLACE CONTRACT: a promotion (promote_begin: the source scan becomes the target) runs this kernel with src == tgt and stride 16 -- the
// records are already packed.  src and tgt therefore carry NO __restrict__, and the body must keep to "thread i reads record i of src, then
// writes record i of tgt": no staging of other threads' records, no reads of a neighbour's record from src (pad sentinels take the thread's
// OWN point p), no vector loads across records.  tests/test_gpu_next_rows.py compares a promoted target with a freshly loaded one bit for bit.
__global__ void __launch_bounds__(256)
target_ingest_kernel(const char* src, int64_t stride, int n, const int* __restrict__ off, int n_rings, int first_ring,
                     float4* tgt, int* __restrict__ ring_of, float4* __restrict__ pad, unsigned* __restrict__ mnmx,
                     unsigned long long* __restrict__ lb_status, int lb_words)
#if VELO_DEF_LOAD
{
    for (int j = blockIdx.x * 256 + threadIdx.x; j < lb_words; j += gridDim.x * 256) lb_status[j] = 0ull;
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
#pragma unroll
    for (int u = 0; u < kIngestPerThread; u++) {
        const int i = (blockIdx.x * kIngestPerThread + u) * 256 + threadIdx.x;
        if (i >= n) continue;
        const float* q = (const float*)(src + (int64_t)i * stride);
        const float4 p = make_float4(q[0], q[1], q[2], 0.0f);
        tgt[i] = p;
        int lo = 0, hi = n_rings;   // find r with off[r] <= i < off[r+1]
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (off[mid] <= i) lo = mid; else hi = mid; }
        ring_of[i] = lo + first_ring;
        const int base = off[lo], end = off[lo + 1];
        pad[i + 2 * lo + 1] = p;
        if (i == base) pad[end + 2 * lo + 1] = p;          // trailing sentinel = first point
        if (i == end - 1) pad[base + 2 * lo] = p;          // leading sentinel = last point
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) {
            mn[0] = fminf(mn[0], p.x); mn[1] = fminf(mn[1], p.y); mn[2] = fminf(mn[2], p.z);
            mx[0] = fmaxf(mx[0], p.x); mx[1] = fmaxf(mx[1], p.y); mx[2] = fmaxf(mx[2], p.z);
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], o));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o));
        }
    }
    __shared__ float red[4][6];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { for (int k = 0; k < 3; k++) { red[wid][k] = mn[k]; red[wid][3 + k] = mx[k]; } }
    __syncthreads();
    if (threadIdx.x < 6) {     // one atomic per workgroup and component, and only where this workgroup moves the box (a stale look is harmless)
        const int k = threadIdx.x;
        float v = red[0][k];
        for (int w = 1; w < 4; w++) v = (k < 3) ? fminf(v, red[w][k]) : fmaxf(v, red[w][k]);
        const unsigned key = f2key(v), cur = mnmx[k];
        if (k < 3) { if (v < 3.0e38f && key < cur) atomicMin(&mnmx[k], key); } else { if (v > -3.0e38f && key > cur) atomicMax(&mnmx[k], key); }
    }
}
#else
;
#endif
__global__ void __launch_bounds__(256)
source_ingest_kernel(const char* __restrict__ raw, int64_t stride, int n, float4* __restrict__ src, int nb_pack,
                     const int* __restrict__ src_off, const int* __restrict__ q_off, int n_rings, int skip, int nq, int patch, int patch_rings, int patch_len,
                     int* __restrict__ q_src, float4* __restrict__ qpts, unsigned* __restrict__ mnmx)
#if VELO_DEF_LOAD
{
    if ((int)blockIdx.x < nb_pack) {
        // (the pack blocks also take the cloud's bounding box -- the keys target_ingest_kernel would compute for the same points: a drive
        //  promotes this scan to target one frame later, and with the box already on the host the index build needs no host wait)
        const int i = blockIdx.x * 256 + threadIdx.x;
        float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
        if (i < n) {
            const float* p = (const float*)(raw + (int64_t)i * stride);
            const float4 v = make_float4(p[0], p[1], p[2], 0.0f);
            src[i] = v;
            if (isfinite(v.x) && isfinite(v.y) && isfinite(v.z)) { mn[0] = mx[0] = v.x; mn[1] = mx[1] = v.y; mn[2] = mx[2] = v.z; }
        }
        if (!mnmx) return;
#pragma unroll
        for (int k = 0; k < 3; k++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
        }
        __shared__ float red[4][6];
        const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
        if (lane == 0) { for (int k = 0; k < 3; k++) { red[wid][k] = mn[k]; red[wid][3 + k] = mx[k]; } }
        __syncthreads();
        if (threadIdx.x < 6) {
            const int k = threadIdx.x;
            float v = red[0][k];
            for (int w = 1; w < 4; w++) v = (k < 3) ? fminf(v, red[w][k]) : fmaxf(v, red[w][k]);
            const unsigned key = f2key(v), cur = mnmx[k];
            if (k < 3) { if (v < 3.0e38f && key < cur) atomicMin(&mnmx[k], key); } else { if (v > -3.0e38f && key > cur) atomicMax(&mnmx[k], key); }
        }
        return;
    }
    const int i = ((int)blockIdx.x - nb_pack) * 256 + threadIdx.x;
    if (i >= nq) return;
    int lo = 0, hi = n_rings;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (q_off[mid] <= i) lo = mid; else hi = mid; }
    const int k = i - q_off[lo];
    const int pos = patch ? patch_position(q_off, n_rings, lo, k, patch_rings, patch_len) : i, si = src_off[lo] + k * skip;
    q_src[pos] = si;
    if (qpts) { const float* p = (const float*)(raw + (int64_t)si * stride); qpts[pos] = make_float4(p[0], p[1], p[2], 0.0f); }
}
#else
;
#endif

// ---- grid build: count, exclusive scan (3 kernels), scatter ----------------------------------------------------
__device__ __forceinline__ int cell_of_point(const GridDesc& g, const float4& p) {
    int cx = cell_coord(p.x, g.ox, g.inv_h, g.nx), cy = cell_coord(p.y, g.oy, g.inv_h, g.ny), cz = cell_coord(p.z, g.oz, g.inv_h, g.nz);
    cx = min(max(cx, 0), g.nx - 1); cy = min(max(cy, 0), g.ny - 1); cz = min(max(cz, 0), g.nz - 1);
    return (cz * g.ny + cy) * g.nx + cx;
}
// The table is built IN PLACE with an offset of one: cell c counts into table[c + 1]; the exclusive scan of table[1..ncells] leaves
// table[c + 1] = start(c); the scatter takes its slots with atomicAdd(&table[c + 1], 1), which leaves table[c + 1] = start(c + 1).
// table[0] stays 0, so in the end table[k] = start(k) for k = 0..ncells -- no cursor copy of the table (a 134 MB write per build
// of the 2M-point map's 33 M cells), no second pass over it.
// Consecutive points of a ring are neighbours in space, on an accumulated map often several per cell: the lanes of a wave that hold a RUN
// of equal cell ids send ONE atomic for the run (count) / take one block of slots for it (scatter).  The atomics on a cell's word come
// from workgroups on different XCDs -- every one moves the line to another L2 -- so fewer of them is what shortens both kernels.
// run_of_lane: `head` lanes start a run; returns the run's first lane and its length (valid on every lane with c >= 0).
__device__ __forceinline__ void run_of_lane(int c, int lane, bool* head, int* first, int* len) {
    const int prev = __shfl_up(c, 1);
    const bool h = c >= 0 && (lane == 0 || prev != c);
    const unsigned long long hm = __ballot(h), vm = __ballot(c >= 0);
    const unsigned long long upto = (2ull << lane) - 1ull;                       // lanes 0..lane
    const int f = 63 - __clzll((long long)((hm & upto) | 1ull));                 // (| 1: keeps clz defined on lanes before the first run)
    const unsigned long long stop = (hm | ~vm) & ~upto;                          // the next run or the next lane without a cell
    *head = h; *first = f; *len = (stop ? (int)__ffsll((long long)stop) - 1 : 64) - f;
}
__global__ void grid_count_kernel(GridDesc g, const float4* __restrict__ pts, int n, int* __restrict__ cell_of, int* __restrict__ table)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int c = -1;
    if (i < n) {
        const float4 p = pts[i];
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) c = cell_of_point(g, p);
        cell_of[i] = c;
    }
    bool head; int first, len;
    run_of_lane(c, threadIdx.x & 63, &head, &first, &len);
    if (head) atomicAdd(&table[c + 1], len);
}
#else
;
#endif

// ---- compressed table (large grids) ----------------------------------------------------------------------------------------------------
// mark: cell id per point (cell_of) + one bit per occupied cell (a run of equal cells sends one atomicOr); word_popc: occupied cells per
// word, ready for the one-pass scan; ccount: every point's COMPACT cell number (its rank among the occupied cells, overwriting cell_of)
// counted into table[k + 1] like grid_count_kernel does for the dense table.  Scan and scatter are the dense path's kernels on the
// compact table: ~8 B per point of table traffic instead of 4 B per CELL read and written twice.
__global__ void grid_mark_kernel(GridDesc g, const float4* __restrict__ pts, int n, int* __restrict__ cell_of, unsigned long long* __restrict__ wmask, int wpr)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int c = -1;
    if (i < n) {
        const float4 p = pts[i];
        if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) c = cell_of_point(g, p);
        cell_of[i] = c;
    }
    bool head; int first, len;
    run_of_lane(c, threadIdx.x & 63, &head, &first, &len);
    if (head) {
        const int row = c / g.nx, x = c - row * g.nx;
        const unsigned long long bit = 1ull << (x & 63);
        unsigned long long* w = &wmask[(size_t)row * wpr + (x >> 6)];
        if (!(__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(w, bit);   // (a set bit stays set: most runs find theirs set already)
    }
}
#else
;
#endif
__global__ void word_popc_kernel(const unsigned long long* __restrict__ wmask, int n_words, int* __restrict__ wprefix)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_words) wprefix[i] = __popcll(wmask[i]);
    else if (i == n_words) wprefix[i] = 0;                              // the sentinel word behind the last row
}
#else
;
#endif
__global__ void grid_ccount_kernel(GridDesc g, int* __restrict__ cell_of, int n, const unsigned long long* __restrict__ wmask, const int* __restrict__ wprefix, int wpr,
                                   int* __restrict__ table)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    int k = -1;
    if (i < n) {
        const int c = cell_of[i];
        if (c >= 0) {
            const int row = c / g.nx, x = c - row * g.nx;
            const int w = row * wpr + (x >> 6);
            k = wprefix[w] + __popcll(wmask[w] & ((1ull << (x & 63)) - 1ull));
        }
        cell_of[i] = k;
    }
    bool head; int first, len;
    run_of_lane(k, threadIdx.x & 63, &head, &first, &len);
    if (head) atomicAdd(&table[k + 1], len);
}
#else
;
#endif

// (kScanThreads / kScanItems / kScanTile and block_exclusive_scan, which the depth rows and the frame kernels use as well: velo_scan_types.h)
// Exclusive scan in ONE pass over the data (decoupled look-back): a workgroup takes the next tile by ticket (so every tile before
// it is already running), scans it locally, publishes its total, and wave 0 looks back over the tiles before it -- 64 status
// words at a time, each {flag, value} in one 64-bit word read with a device-scope atomic -- adding totals until it meets a tile
// whose whole prefix is known.  The atomics are RELAXED on purpose: a status word carries everything its reader needs, and an
// acquire / release at device scope costs an L2 invalidate / write-back per spin (measured: the whole chip slows down 2x).  Read once, write once: 2 x 134 MB for the map's table instead of 5 x (three-kernel scan + cursor).
// Elements per thread and tile: 16 (4,096-element tiles) for a scan's table, 64 (16,384) for a map's -- the one-pass scan is bound by its
// NUMBER of tiles (ticket, status word, look-back per tile), not by bytes: on the 23 M cells of the 2M-point map 1,024-element tiles take
// 272 us, 4,096: 96 us, 8,192: 67 us, 16,384: 56 us (185 MB: 3.3 TB/s); on the 0.87 M cells of a scan 16,384-element tiles leave 53
// workgroups for the chip (11.0 against 7.9 us).
constexpr int kLbItemsSmall = 16, kLbItemsLarge = 64;
constexpr int kLbLargeFrom = 1 << 22;              // table entries from which the large tiles are used
__host__ __device__ constexpr int lb_tile(int items) { return kScanThreads * items; }
constexpr unsigned long long kLbAgg = 1ull << 62, kLbPrefix = 2ull << 62, kLbFlags = 3ull << 62;
template <int kLbItems>
__device__ __forceinline__ void
scan_lookback_body(int* __restrict__ data, int n, unsigned long long* __restrict__ status, int* __restrict__ ticket, int* __restrict__ grand_total) {
    // A tile = kLbItems / 4 sub-tiles of kScanThreads x 4 ints; thread t holds the int4 number t of EVERY sub-tile, so a wave's loads and
    // stores are 1 KB of consecutive memory.  The sub-tiles' prefixes come out of ONE round of wave scans (all sub-tiles at once) and
    // one barrier.
    constexpr int kSub = kLbItems / 4, kWaves = kScanThreads / kWave, kLbTile = lb_tile(kLbItems);
    static_assert(kLbItems % 4 == 0, "int4 loads");
    __shared__ int s_tile, s_prefix;
    __shared__ int s_wsum[kSub][kWaves];
    if (threadIdx.x == 0) s_tile = atomicAdd(ticket, 1);
    __syncthreads();
    const int tile = s_tile;
    const int tbase = tile * kLbTile, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int4 v[kSub];
    int inc[kSub];
#pragma unroll
    for (int k = 0; k < kSub; k++) {
        const int i = tbase + k * (kScanThreads * 4) + threadIdx.x * 4;
        if (i + 3 < n) v[k] = *reinterpret_cast<const int4*>(data + i);
        else { v[k].x = i < n ? data[i] : 0; v[k].y = i + 1 < n ? data[i + 1] : 0; v[k].z = i + 2 < n ? data[i + 2] : 0; v[k].w = 0; }
        inc[k] = (v[k].x + v[k].y) + (v[k].z + v[k].w);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < kSub; k++) { const int t = __shfl_up(inc[k], off); if (lane >= off) inc[k] += t; }
    }
    if (lane == 63) {
#pragma unroll
        for (int k = 0; k < kSub; k++) s_wsum[k][wid] = inc[k];
    }
    __syncthreads();
    int ex[kSub], run = 0;                                              // exclusive prefix of this thread's int4 inside the tile
#pragma unroll
    for (int k = 0; k < kSub; k++) {
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) { const int sw = s_wsum[k][w]; if (w < wid) before += sw; all += sw; }
        ex[k] = run + before + inc[k] - ((v[k].x + v[k].y) + (v[k].z + v[k].w));
        run += all;
    }
    const int total = run;
    if (threadIdx.x == 0) {
        s_prefix = 0;
        __hip_atomic_store(&status[tile], (tile == 0 ? kLbPrefix : kLbAgg) | (unsigned long long)(unsigned)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (tile > 0 && threadIdx.x < 64) {
        int acc = 0;
        for (int idx = tile - 1;; idx -= 64) {
            const int j = idx - lane;                                  // lane 0 = the nearest tile before this one
            unsigned long long w = kLbPrefix;                          // tiles before the first: prefix 0
            if (j >= 0) { do { w = __hip_atomic_load(&status[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((w & kLbFlags) == 0ull); }
            const unsigned long long pm = __ballot((w & kLbFlags) == kLbPrefix);
            const int first = (int)__ffsll((long long)pm) - 1;         // pm != 0 at the latest when j < 0 appears
            int val = (pm == 0ull || lane <= first) ? (int)(unsigned)(w & 0xffffffffull) : 0;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) val += __shfl_xor(val, off);
            acc += val;
            if (pm != 0ull) break;
        }
        if (lane == 0) {
            s_prefix = acc;
            __hip_atomic_store(&status[tile], kLbPrefix | (unsigned long long)(unsigned)(acc + total), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __syncthreads();
    const int pre = s_prefix;
#pragma unroll
    for (int k = 0; k < kSub; k++) {
        const int i = tbase + k * (kScanThreads * 4) + threadIdx.x * 4;
        int4 q;
        q.x = pre + ex[k]; q.y = q.x + v[k].x; q.z = q.y + v[k].y; q.w = q.z + v[k].z;
        if (i + 3 < n) *reinterpret_cast<int4*>(data + i) = q;
        else { if (i < n) data[i] = q.x; if (i + 1 < n) data[i + 1] = q.y; if (i + 2 < n) data[i + 2] = q.z; }
        if (i <= n - 1 && n - 1 < i + 4) *grand_total = q.w + v[k].w;  // the thread that holds the last element: its running sum is the total (elements beyond n are zero)
    }
}
template <int kLbItems>
__global__ void __launch_bounds__(kScanThreads)
scan_lookback_kernel(int* __restrict__ data, int n, unsigned long long* __restrict__ status, int* __restrict__ ticket, int* __restrict__ grand_total) {
    scan_lookback_body<kLbItems>(data, n, status, ticket, grand_total);
}
// (three-kernel scan, kept for the device ring segmenter's small arrays)
// pass 1: tile-local exclusive scan in place (counts -> local offsets), tile totals out
__global__ void scan_tiles_kernel(int* __restrict__ data, int n, int* __restrict__ tile_sums)
#if VELO_DEF_LOAD
{
    const int base = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    int v[kScanItems], s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; k++) { v[k] = (base + k < n) ? data[base + k] : 0; s += v[k]; }
    int total;
    int ex = block_exclusive_scan(s, &total);
#pragma unroll
    for (int k = 0; k < kScanItems; k++) { if (base + k < n) data[base + k] = ex; ex += v[k]; }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}
#else
;
#endif
// pass 2: one workgroup scans the tile totals in place (exclusive) and writes the grand total to data_total
__global__ void scan_sums_kernel(int* __restrict__ tile_sums, int n_tiles, int* __restrict__ grand_total)
#if VELO_DEF_LOAD
{
    __shared__ int carry_s;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int start = 0; start < n_tiles; start += kScanThreads) {
        const int i = start + threadIdx.x;
        const int v = (i < n_tiles) ? tile_sums[i] : 0;
        int total;
        const int ex = block_exclusive_scan(v, &total);
        const int carry = carry_s;
        if (i < n_tiles) tile_sums[i] = ex + carry;
        __syncthreads();
        if (threadIdx.x == 0) carry_s = carry + total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *grand_total = carry_s;
}
#else
;
#endif
// pass 3: add tile offsets; also seed the scatter cursor; element n receives the grand total
__global__ void scan_add_kernel(int* __restrict__ data, int n, const int* __restrict__ tile_sums, const int* __restrict__ grand_total,
                                int* __restrict__ cursor)
#if VELO_DEF_LOAD
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { const int v = data[i] + tile_sums[i / kScanTile]; data[i] = v; cursor[i] = v; }
    else if (i == n) data[n] = *grand_total;
}
#else
;
#endif
__device__ __forceinline__ void grid_scatter_body(const float4* __restrict__ pts, const int* __restrict__ cell_of, const int* __restrict__ ring_of, int n,
                                                  int* __restrict__ cursor, const int* __restrict__ n_finite, int first_point,
                                                  float4* __restrict__ sorted, int* __restrict__ sring, const int bx) {
    const int i = bx * 256 + threadIdx.x;
    if (i < kGridPad) {   // sentinels behind the last real point: +inf coordinates can never pass the gate
        const int j = *n_finite + i;
        sorted[j] = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), __int_as_float(0x7fffffff));
        sring[j] = 0x7fffffff;
    }
    const int c = i < n ? cell_of[i] : -1;
    bool head; int first, len;
    const int lane = threadIdx.x & 63;
    run_of_lane(c, lane, &head, &first, &len);
    int slot = head ? atomicAdd(&cursor[c], len) : 0;                  // cursor = table + 1 (see grid_count_kernel); one block of slots per run
    slot = __shfl(slot, first) + (lane - first);
    if (c < 0) return;
    const float4 p = pts[i];
    sorted[slot] = make_float4(p.x, p.y, p.z, __int_as_float(i + first_point));
    sring[slot] = ring_of[i];
}
__global__ void __launch_bounds__(256)
grid_scatter_kernel(const float4* __restrict__ pts, const int* __restrict__ cell_of, const int* __restrict__ ring_of, int n,
                    int* __restrict__ cursor, const int* __restrict__ n_finite, int first_point, float4* __restrict__ sorted, int* __restrict__ sring)
#if VELO_DEF_LOAD
{
    grid_scatter_body(pts, cell_of, ring_of, n, cursor, n_finite, first_point, sorted, sring, (int)blockIdx.x);
}
#else
;
#endif

// ---- the next frame of a drive in three launches for a whole lock-step group (velo_hint_next_frame) -------------------------------------
// A drive's step loads a frame on both sides: the scan the context holds as source becomes the target (ring ids, padded rings, index), the
// announced scan becomes the source (packed copy, query list, bounding box).  Through the general loaders that is thirteen queue operations
// per context -- two ring-table copies, ingest, count, scan, scatter, source ingest, the box's way back, fills -- at 5-10 us of hand-over
// each with four busy queues: 170-290 us on the stream for a group of two, as long as the host takes to turn a step around.  Here the jobs
// of ALL contexts of a group ride in the kernel arguments (ring tables included: up to kAdvRings rings), and the stages that do not depend
// on each other share a launch:
//   advance_ingest_kernel   target side: ring ids + padded rings of the (already packed) promoted cloud, cell ids and the cells' counts
//                           (the box is known from the frame's time as source, so the grid is sized before anything runs);
//                           source side: source_ingest_kernel's work; both sides' ring tables written for the kernels that follow
//   advance_scan_kernel     the one-pass scan of every context's table
//   advance_scatter_kernel  the cell-sorted copies
// Same arithmetic and the same tables as the general loaders, which every other entry keeps using (tests compare the two bit for bit).
constexpr int kAdvRings = 64, kAdvJobs = 4;
struct AdvJob {
    // target side
    const float4* tgt; int* tgt_off_dev; int* ring_of; float4* pad; unsigned long long* lb_status; int* cell_of; int* table;
    float4* sorted; int* sring; int* scan_total; int* lb_ticket; int* clear; int n_clear;   // clear: the index table's words, zeroed ahead of the counts
    GridDesc g;
    int n_t, n_rings_t, first_ring, first_point, lb_words, nb_t, nc, n_tiles, nb_sc;
    // source side
    const char* raw; long long stride; float4* src; int* src_off_dev; int* q_src; float4* qpts; unsigned* keys; unsigned* keys_next;
    unsigned* h_keys;                                                   // page-locked host memory: the source's box keys ride back with the last launch
    float4* seed_fill;                                                  // both winners' seed arrays (2 nq entries) set to "none" here, or null
    int n_s, n_rings_s, nb_pack, nb_q, skip, nq, patch, patch_rings, patch_len;
    int off_t[kAdvRings + 1], off_s[kAdvRings + 1];
};
struct AdvBatch { AdvJob job[kAdvJobs]; };

// every context's index table zeroed in one launch (the runtime's fill is a queue operation per table)
__global__ void __launch_bounds__(256)
advance_clear_kernel(AdvBatch B)
#if VELO_DEF_LOAD
{
    const AdvJob& J = B.job[blockIdx.y];
    int4* p = reinterpret_cast<int4*>(J.clear);                        // (hipMalloc'd: 256-byte aligned; n_clear rounded up to whole int4s by the host, inside the allocation)
    const int n4 = J.n_clear >> 2;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256) p[i] = make_int4(0, 0, 0, 0);
}
#else
;
#endif
__global__ void __launch_bounds__(256)
advance_ingest_kernel(AdvBatch B)
#if VELO_DEF_LOAD
{
    const AdvJob& J = B.job[blockIdx.y];
    __shared__ int s_off[kAdvRings + 2], s_qoff[kAdvRings + 2];
    __shared__ float red[4][6];
    const int tid = threadIdx.x, lane = tid & 63;
    int bx = blockIdx.x;
    if (bx < J.nb_t) {
        // ---- target side: target_ingest_kernel on a packed cloud in place (nothing to pack, box known) + grid_count_kernel ----
        const int R = J.n_rings_t, n = J.n_t;
        if (tid <= R) s_off[tid] = J.off_t[tid];
        for (int j = bx * 256 + tid; j < J.lb_words; j += J.nb_t * 256) J.lb_status[j] = 0ull;
        __syncthreads();
        if (bx == 0 && tid <= R) J.tgt_off_dev[tid] = s_off[tid];
#pragma unroll
        for (int u = 0; u < kIngestPerThread; u++) {
            const int i = (bx * kIngestPerThread + u) * 256 + tid;
            int c = -1;
            if (i < n) {
                const float4 p = J.tgt[i];
                int lo = 0, hi = R;   // find r with off[r] <= i < off[r+1]
                while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] <= i) lo = mid; else hi = mid; }
                J.ring_of[i] = lo + J.first_ring;
                const int base = s_off[lo], end = s_off[lo + 1];
                J.pad[i + 2 * lo + 1] = p;
                if (i == base) J.pad[end + 2 * lo + 1] = p;          // trailing sentinel = first point
                if (i == end - 1) J.pad[base + 2 * lo] = p;          // leading sentinel = last point
                if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z)) c = cell_of_point(J.g, p);
                J.cell_of[i] = c;
            }
            bool head; int first, len;
            run_of_lane(c, lane, &head, &first, &len);
            if (head) atomicAdd(&J.table[c + 1], len);
        }
        return;
    }
    bx -= J.nb_t;
    if (bx >= J.nb_pack) return;
    // ---- source side: source_ingest_kernel, ring and query tables from the arguments ----
    const int R = J.n_rings_s;
    if (tid <= R) s_off[tid] = J.off_s[tid];
    if (tid < 64) {                                                    // query offsets: smi = 0, skip, 2 skip, ... < n per ring (velo.h:807)
        int cnt = tid < R ? (J.off_s[tid + 1] - J.off_s[tid] + J.skip - 1) / J.skip : 0;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(cnt, o); if (lane >= o) cnt += t; }
        if (tid == 0) s_qoff[0] = 0;
        if (tid < R) s_qoff[tid + 1] = cnt;
    }
    __syncthreads();
    if (bx == 0) {
        if (tid <= R) { J.src_off_dev[tid] = s_off[tid]; J.src_off_dev[R + 1 + tid] = s_qoff[tid]; }
        if (tid < 6) J.keys_next[tid] = tid < 3 ? 0xffffffffu : 0u;     // the keys of the frame after this one (the two slots alternate)
    }
    if (bx >= J.nb_pack) return;
    // ONE pass over the caller's records: the workgroup's 256 records come in with 16-byte loads where the layout allows (stride 12: 3 KB
    // of consecutive bytes through LDS; stride 16: one load per record) -- the records may live in page-locked HOST memory, where every
    // load instruction is a trip over the bus -- and the thread that packs point i also emits its query: ring r, every skip-th point
    // (velo.h:807) -> position in the (patch-ordered) list, the same map source_ingest_kernel's query blocks walk from the other side.
    __shared__ float s_raw[256 * 3];
    const int i = bx * 256 + tid;
    const bool have = i < J.n_s;
    const bool aligned = (reinterpret_cast<unsigned long long>(J.raw) & 15ull) == 0ull;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (J.stride == 12 && aligned) {
        const char* base = J.raw + (long long)bx * 3072;
        const int nbytes = min(3072, (J.n_s - bx * 256) * 12);
        if (tid < 192) {
            if (tid * 16 + 16 <= nbytes) *reinterpret_cast<uint4*>(&s_raw[tid * 4]) = *reinterpret_cast<const uint4*>(base + tid * 16);
            else for (int f = 0; f < 4; f++) if (tid * 16 + 4 * f + 4 <= nbytes) s_raw[tid * 4 + f] = *reinterpret_cast<const float*>(base + tid * 16 + 4 * f);
        }
        __syncthreads();
        if (have) v = make_float4(s_raw[3 * tid], s_raw[3 * tid + 1], s_raw[3 * tid + 2], 0.0f);
    } else if (have) {
        const char* q = J.raw + (long long)i * J.stride;
        if (J.stride == 16 && aligned) { const float4 w = *reinterpret_cast<const float4*>(q); v = make_float4(w.x, w.y, w.z, 0.0f); }
        else { const float* p = reinterpret_cast<const float*>(q); v = make_float4(p[0], p[1], p[2], 0.0f); }
    }
    float mn[3] = {3.0e38f, 3.0e38f, 3.0e38f}, mx[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    if (have) {
        J.src[i] = v;
        if (isfinite(v.x) && isfinite(v.y) && isfinite(v.z)) { mn[0] = mx[0] = v.x; mn[1] = mx[1] = v.y; mn[2] = mx[2] = v.z; }
        if (J.nq > 0) {
            int lo = 0, hi = R;                                            // ring of point i
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (s_off[mid] <= i) lo = mid; else hi = mid; }
            const int j = i - s_off[lo];
            if (j % J.skip == 0) {
                const int k = j / J.skip;
                const int pos = J.patch ? patch_position(s_qoff, R, lo, k, J.patch_rings, J.patch_len) : s_qoff[lo] + k;
                J.q_src[pos] = i;
                if (J.qpts) J.qpts[pos] = v;
                if (J.seed_fill) {                                     // (what attach_seeds' fill of 0xff bytes writes: no previous winner)
                    const float4 none = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1));
                    J.seed_fill[pos] = none; J.seed_fill[J.nq + pos] = none;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mn[k] = fminf(mn[k], __shfl_xor(mn[k], o)); mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], o)); }
    }
    const int wid = tid >> 6;
    if (lane == 0) { for (int k = 0; k < 3; k++) { red[wid][k] = mn[k]; red[wid][3 + k] = mx[k]; } }
    __syncthreads();
    if (tid < 6) {
        const int k = tid;
        float vv = red[0][k];
        for (int w = 1; w < 4; w++) vv = (k < 3) ? fminf(vv, red[w][k]) : fmaxf(vv, red[w][k]);
        const unsigned key = f2key(vv), cur = J.keys[k];
        if (k < 3) { if (vv < 3.0e38f && key < cur) atomicMin(&J.keys[k], key); } else { if (vv > -3.0e38f && key > cur) atomicMax(&J.keys[k], key); }
    }
}
#else
;
#endif
template <int kLbItems>
__global__ void __launch_bounds__(kScanThreads)
advance_scan_kernel(AdvBatch B) {
    const AdvJob& J = B.job[blockIdx.y];
    if ((int)blockIdx.x >= J.n_tiles) return;
    scan_lookback_body<kLbItems>(J.table + 1, J.nc, J.lb_status, J.lb_ticket, J.scan_total);
}
__global__ void __launch_bounds__(256)
advance_scatter_kernel(AdvBatch B)
#if VELO_DEF_LOAD
{
    const AdvJob& J = B.job[blockIdx.y];
    if ((int)blockIdx.x >= J.nb_sc) return;
    // (the source's bounding box, complete since the ingest launch ended, written where the host reads it before the scan's promotion one
    //  step later: two copies per group and step less)
    if (blockIdx.x == 0 && threadIdx.x < 6 && J.h_keys) J.h_keys[threadIdx.x] = J.keys[threadIdx.x];
    grid_scatter_body(J.tgt, J.cell_of, J.ring_of, J.n_t, J.table + 1, J.scan_total, J.first_point, J.sorted, J.sring, (int)blockIdx.x);
}
#else
;
#endif

// ---- template kernels: instantiated by the unit that owns the family, `extern template` for everybody else --------------------------------
#if VELO_DEF_LOAD
#define VELO_INST_LOAD template
#else
#define VELO_INST_LOAD extern template
#endif
VELO_INST_LOAD __global__ void scan_lookback_kernel<kLbItemsSmall>(int*, int, unsigned long long*, int*, int*);
VELO_INST_LOAD __global__ void scan_lookback_kernel<kLbItemsLarge>(int*, int, unsigned long long*, int*, int*);
VELO_INST_LOAD __global__ void advance_scan_kernel<kLbItemsSmall>(AdvBatch);
VELO_INST_LOAD __global__ void advance_scan_kernel<kLbItemsLarge>(AdvBatch);

}  // namespace velo
