// velo_frame_kernels.h -- frameToFrame's visual matches assembled on the device from resident keypoint frames: matchUsingId
// (reference velo.h:562-590), the landmark substitution (velo.h:634-644) and the gather of a match's operands (velo.h:645-654).
// Included by velo_hip.hip (declarations) and by velo_unit_frames.hip (VELO_DEF_FRAMES: the definitions); gfx950 only.
//
// What a context keeps on the device (velo_api_frames.inl owns the buffers): an arena of 4-byte words in which every (frame, camera)
// put so far owns one block  ids[n] | has_depth[n] | keypoints[n][2] | kp_with_depth[n_with_depth][3],  and one slot table per camera,
// slots[cam][id] = -1 between calls.  A call is four launches for all contexts and cameras it names (a UNIT is one camera of one
// context, read from a device table at a workgroup-uniform index):
//     fr_fill_kernel    slots[id] = the LAST index of frame1 that holds id (atomicMax: whatever the thread order)
//     fr_count_kernel   per chunk of kFrChunk entries of frame2: how many of their ids frame1 holds
//     fr_emit_kernel    a chunk's first record = the matches of the context's chunks before it (cameras in order, ind2 ascending); inside
//                       the chunk a workgroup scan keeps ind2 order; every match writes its 68-byte record and its (point1, point2) pair
//     fr_clear_kernel   walks frame1's ids again and sets their slots back to -1: no cost depends on the size of the id space
//
// The loop-closure edge (matchFeatures in place of matchUsingId, main.cpp:359) joins the two frames by their descriptor rows instead:
// the match kernels (velo_match_kernels.h) leave every camera's kept (queryIdx, trainIdx) pairs in query order and their count, and
//     fr_emit_desc_kernel   one thread per kept pair writes the same record; a record's position is the kept counts of the context's
//                           earlier cameras plus the pair's rank in its camera, read from the filter's output (no counter, no atomics)
//
// A registration's good matches prune the current frame (removeSlightlyLessTerribleFeatures, velo.h:272-327): every (frame, camera)
// block is cut down to the keypoints that occur as point1 of a record the gate flagged -- a mark, a scan and a scatter, no arithmetic:
//     fr_mark_kernel          one thread per record of a context's visual set (or per entry of a keep list): map[point1] = 1, a plain
//                             byte store of the same value whoever wins; the map is cleared on the stream before the launch
//     fr_prune_count_kernel   per chunk of kFrChunk keypoints: kept keypoints | kept keypoints with depth << 16 (one packed scan)
//     fr_prune_move_kernel    a chunk's first kept keypoint = the kept ones of the unit's earlier chunks, inside the chunk the packed scan
//                             keeps index order (no counter: the order is fixed); writes the block in the layout of the NEW n, the kept
//                             old indices and the kept descriptor rows
// The new layout overlaps the old one (has_depth starts at word m, inside the old ids) while other workgroups still read the old block,
// so the move kernel never writes an arena: it gathers into scratch that nothing else of the launch reads, and the host copies a unit's
// result over its block in stream order (velo_api_frames.inl), after the whole launch.
//
// A frame put with its keypoint depth (velo_frames_put_frame[_batch]: projectLidarToCamera + featureDepthAssociation, velo.h:329-497,
// in front of the store): the bodies are velo_depth_kernels.h's device functions, run per UNIT on stacks of the frame store's own,
//     fr_depth_project_kernel   grid (rings, units): project_ring on the unit's cloud, window and stacks
//     fr_depth_assoc_kernel     one wave per keypoint of every unit: depth_assoc_keypoint -> the keypoint's point and flag
//     fr_depth_count_kernel     per chunk of kFrChunk keypoints: how many have depth
//     fr_depth_write_kernel     a chunk's first depth point = those of the unit's earlier chunks, inside the chunk the scan keeps
//                               keypoint order (no counter: velo.h:481-483's append order); writes has_depth and the cloud into the
//                               unit's block image, whose ids and keypoints came with the call's upload
//     fr_depth_obs_kernel       (VELO_PUT_OBSERVE) one thread per keypoint: the image's entry as lm_append_kernel's record and id
// The image is sized for n depth points and lies in scratch: the host learns the count, places the block at its exact size and copies.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/velo_hip.h"
#include "velo_scan_types.h"
#include "velo_depth_kernels.h"
#include "velo_landmark_kernels.h"

#ifndef VELO_DEF_FRAMES
#define VELO_DEF_FRAMES 0
#endif

namespace velo {

constexpr int kFrChunk = 256;          // entries of frame2 per workgroup: one per thread of the compaction's scan (kScanThreads)

// one (frame, camera) block of the arena
struct FrSide {
    const int* ids;
    const int* has_depth;
    const float* xy;
    const float* cloud;
    int n, pad;
};

// one camera of one context of a call
struct FrUnit {
    FrSide f1, f2;
    int* slots;                        // this camera's slot table, slot_ids entries
    int slot_ids;
    int ctx, cam;
    int chunk0;                        // index of this unit's first chunk in the call's count array ...
    int ctx_chunk0;                    // ... and of the first chunk of its context's camera 0
    float t_cam[3];
};

// one context of a call: where its records go and where its landmarks are
struct FrCtx {
    VisualMatch* vm;
    int* pairs;                        // (point1, point2) per record, in record order
    const float* lm_pts;               // null: no substitution (no landmark store, or no pose given)
    const unsigned char* lm_added;
    int lm_ids, pad;
    LmPose pose2_inv;
};

__global__ void __launch_bounds__(256)
fr_fill_kernel(const FrUnit* __restrict__ units)
#if VELO_DEF_FRAMES
{
    const FrUnit& U = units[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U.f1.n) return;
    const int id = U.f1.ids[i];
    if (id >= 0 && id < U.slot_ids) atomicMax(U.slots + id, i);      // velo.h:571-574: a later index overwrites an earlier one
}
#else
;
#endif

__global__ void __launch_bounds__(256)
fr_clear_kernel(const FrUnit* __restrict__ units)
#if VELO_DEF_FRAMES
{
    const FrUnit& U = units[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U.f1.n) return;
    const int id = U.f1.ids[i];
    if (id >= 0 && id < U.slot_ids) U.slots[id] = -1;
}
#else
;
#endif

// one camera of one context of a descriptor-matched call; unit u is match job u of the call
struct FrDescUnit {
    FrSide f1, f2;                     // f1 = the query side (the current frame), f2 = the train side
    int ctx, cam;
    int ctx_unit0;                     // the unit of this context's camera 0
    int q_out;                         // first entry of this unit's job in the filter's per-query outputs
    float t_cam[3];
    int pad;
};

// the record of the match (ind1, ind2) of one camera (velo.h:630-654) and its pair, written at position pos of the context's visual set
template <typename Unit>
__device__ __forceinline__ void fr_write_record(const Unit& U, const FrCtx& C, int ind1, int ind2, int pos) {
    const FrSide& f1 = U.f1;
    const FrSide& f2 = U.f2;
    static_assert(sizeof(VisualMatch) == 13 * sizeof(float) + 3 * sizeof(int) + 4, "no padding between the members: zeroing them zeroes the record");
    VisualMatch m = {};                                               // every byte that is not written below is zero, pad included
    const int id = f2.ids[ind2];
    const int h1 = f1.has_depth[ind1], h2 = f2.has_depth[ind2];
    bool d2 = h2 != -1;                                               // velo.h:631-632
    if (C.lm_pts != nullptr && id < C.lm_ids && C.lm_added[id] != 0) {  // velo.h:634-644: landmarks_at_frame.count(id)
        lm_move_point(C.lm_pts + 3 * (size_t)id, C.pose2_inv.m, m.p3_2);
        d2 = true;
    } else if (d2) {                                                  // velo.h:645-648
        const float* p = f2.cloud + 3 * (size_t)h2;
        m.p3_2[0] = p[0]; m.p3_2[1] = p[1]; m.p3_2[2] = p[2];
    }
    if (h1 != -1) {                                                   // velo.h:649-652
        const float* p = f1.cloud + 3 * (size_t)h1;
        m.p3_1[0] = p[0]; m.p3_1[1] = p[1]; m.p3_1[2] = p[2];
    }
    m.p2_1[0] = f1.xy[2 * (size_t)ind1]; m.p2_1[1] = f1.xy[2 * (size_t)ind1 + 1];     // velo.h:653-654
    m.p2_2[0] = f2.xy[2 * (size_t)ind2]; m.p2_2[1] = f2.xy[2 * (size_t)ind2 + 1];
    m.t_cam[0] = U.t_cam[0]; m.t_cam[1] = U.t_cam[1]; m.t_cam[2] = U.t_cam[2];
    m.cam = U.cam; m.point1 = ind1; m.point2 = ind2;
    m.d1 = h1 != -1 ? 1 : 0; m.d2 = d2 ? 1 : 0;
    C.vm[pos] = m;
    C.pairs[2 * (size_t)pos] = ind1;
    C.pairs[2 * (size_t)pos + 1] = ind2;
}

// the index of frame1 that entry ind2 of frame2 matches, or -1 (velo.h:575-579)
__device__ __forceinline__ int fr_lookup(const FrUnit& U, int ind2) {
    if (ind2 >= U.f2.n) return -1;
    const int id = U.f2.ids[ind2];
    return (id >= 0 && id < U.slot_ids) ? U.slots[id] : -1;
}

__global__ void __launch_bounds__(kFrChunk)
fr_count_kernel(const FrUnit* __restrict__ units, int* __restrict__ counts)
#if VELO_DEF_FRAMES
{
    const FrUnit& U = units[blockIdx.y];
    const int first = blockIdx.x * kFrChunk;
    if (first >= U.f2.n) return;                                      // workgroup-uniform
    const int hit = fr_lookup(U, first + (int)threadIdx.x) >= 0 ? 1 : 0;
    int total;
    (void)block_exclusive_scan(hit, &total);
    if (threadIdx.x == 0) counts[U.chunk0 + blockIdx.x] = total;
}
#else
;
#endif

__global__ void __launch_bounds__(kFrChunk)
fr_emit_kernel(const FrUnit* __restrict__ units, const FrCtx* __restrict__ ctxs, const int* __restrict__ counts)
#if VELO_DEF_FRAMES
{
    __shared__ int part[kFrChunk / kWave];
    const FrUnit& U = units[blockIdx.y];
    const int first = blockIdx.x * kFrChunk;
    if (first >= U.f2.n) return;                                      // workgroup-uniform
    const FrCtx& C = ctxs[U.ctx];
    // records of the context's chunks before this one: earlier cameras, then earlier chunks of this camera
    const int mine = U.chunk0 + blockIdx.x;
    int before = 0;
    for (int k = U.ctx_chunk0 + (int)threadIdx.x; k < mine; k += kFrChunk) before += counts[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = before;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < kFrChunk / kWave; w++) base += part[w];
    const int ind2 = first + (int)threadIdx.x;
    const int ind1 = fr_lookup(U, ind2);
    int total;
    const int pos = base + block_exclusive_scan(ind1 >= 0 ? 1 : 0, &total);
    if (ind1 < 0) return;
    fr_write_record(U, C, ind1, ind2, pos);
}
#else
;
#endif

// job_out: the filter's per-job {min_dist, n_kept}; pairs: its kept (queryIdx, trainIdx) pairs, job j's from entry q_out
__global__ void __launch_bounds__(256)
fr_emit_desc_kernel(const FrDescUnit* __restrict__ units, const FrCtx* __restrict__ ctxs, const int* __restrict__ job_out,
                    const int* __restrict__ pairs)
#if VELO_DEF_FRAMES
{
    const int u = blockIdx.y;
    const FrDescUnit& U = units[u];
    const int kept = job_out[2 * u + 1];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= kept) return;
    int base = 0;                                                     // at most 7 earlier cameras, workgroup-uniform
    for (int v = U.ctx_unit0; v < u; v++) base += job_out[2 * v + 1];
    const int* pr = pairs + 2 * ((size_t)U.q_out + (size_t)k);
    fr_write_record(U, ctxs[U.ctx], pr[0], pr[1], base + k);
}
#else
;
#endif

// one camera of one context of a prune call (or the one entry of velo_frames_keep)
struct FrPruneUnit {
    FrSide f;                          // the entry as it is: read only
    const uint4* rows;                 // its descriptor rows, four uint4 each, or null
    unsigned char* map;                // f.n bytes, 1 = the keypoint stays
    int* out;                          // scratch, 64-byte aligned: ids[m] | has_depth[m] | xy[m][2] | cloud[m_with_depth][3] for the new m
    uint4* rows_out;                   // scratch: the kept rows
    int* kept;                         // the kept old indices, ascending
    int chunk0, n_chunks;              // this unit's chunks in the call's count array
};

// what marks: the visual set of one context (its units are unit0 + cam), or a keep list for unit0
struct FrPruneSrc {
    const VisualMatch* vm;
    const unsigned char* vflags;       // three slots per record; a record counts when any is non-zero
    const int* keep;                   // non-null: n indices instead of records
    int n, unit0, n_cams, pad;
};

__global__ void __launch_bounds__(256)
fr_mark_kernel(const FrPruneUnit* __restrict__ units, const FrPruneSrc* __restrict__ srcs)
#if VELO_DEF_FRAMES
{
    const FrPruneSrc& S = srcs[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    int u = S.unit0, idx;
    if (S.keep != nullptr) idx = S.keep[i];
    else {
        const unsigned char* f = S.vflags + 3 * (size_t)i;
        if ((f[0] | f[1] | f[2]) == 0) return;                        // velo_get_good_matches reports a record once per non-zero slot
        const int cam = S.vm[i].cam;
        if (cam < 0 || cam >= S.n_cams) return;
        u += cam;
        idx = S.vm[i].point1;
    }
    const FrPruneUnit& U = units[u];
    if (idx >= 0 && idx < U.f.n) U.map[idx] = 1;                      // the std::set of velo.h:287-290: idempotent, no atomics
}
#else
;
#endif

// kept | kept-with-depth << 16 of keypoint i of U: both at most kFrChunk per chunk, so the packed sums never carry
__device__ __forceinline__ int fr_prune_flag(const FrPruneUnit& U, int i, int* has_depth) {
    *has_depth = -1;
    if (i >= U.f.n || U.map[i] == 0) return 0;
    *has_depth = U.f.has_depth[i];
    return *has_depth != -1 ? 0x10001 : 1;
}

__global__ void __launch_bounds__(kFrChunk)
fr_prune_count_kernel(const FrPruneUnit* __restrict__ units, int* __restrict__ counts)
#if VELO_DEF_FRAMES
{
    const FrPruneUnit& U = units[blockIdx.y];
    const int first = blockIdx.x * kFrChunk;
    if (first >= U.f.n) return;                                       // workgroup-uniform
    int d, total;
    (void)block_exclusive_scan(fr_prune_flag(U, first + (int)threadIdx.x, &d), &total);
    if (threadIdx.x == 0) counts[U.chunk0 + blockIdx.x] = total;
}
#else
;
#endif

__global__ void __launch_bounds__(kFrChunk)
fr_prune_move_kernel(const FrPruneUnit* __restrict__ units, const int* __restrict__ counts)
#if VELO_DEF_FRAMES
{
    __shared__ int part[3][kFrChunk / kWave];
    __shared__ int src[kFrChunk];
    const FrPruneUnit& U = units[blockIdx.y];
    const int first = blockIdx.x * kFrChunk;
    if (first >= U.f.n) return;                                       // workgroup-uniform
    // the unit's kept keypoints (the new n) and what its chunks before this one keep, with and without depth
    int all = 0, bk = 0, bd = 0;
    for (int k = (int)threadIdx.x; k < U.n_chunks; k += kFrChunk) {
        const int c = counts[U.chunk0 + k];
        all += c & 0xffff;
        if (k < (int)blockIdx.x) { bk += c & 0xffff; bd += c >> 16; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { all += __shfl_xor(all, off); bk += __shfl_xor(bk, off); bd += __shfl_xor(bd, off); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = all; part[1][threadIdx.x >> 6] = bk; part[2][threadIdx.x >> 6] = bd; }
    __syncthreads();
    int m = 0, base = 0, base_d = 0;
#pragma unroll
    for (int w = 0; w < kFrChunk / kWave; w++) { m += part[0][w]; base += part[1][w]; base_d += part[2][w]; }
    const int i = first + (int)threadIdx.x;
    int d, total;
    const int flag = fr_prune_flag(U, i, &d);
    const int ex = block_exclusive_scan(flag, &total);
    if (flag != 0) {                                                  // velo.h:303-317, j and jd from the scan
        const int j = base + (ex & 0xffff);
        int* o = U.out;
        o[j] = U.f.ids[i];
        reinterpret_cast<float2*>(o + 2 * (size_t)m)[j] = reinterpret_cast<const float2*>(U.f.xy)[i];
        if (d != -1) {
            const int jd = base_d + (ex >> 16);
            const float* p = U.f.cloud + 3 * (size_t)d;               // a depth point two keypoints share is copied for each
            float* q = reinterpret_cast<float*>(o + 4 * (size_t)m) + 3 * (size_t)jd;
            q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
            o[(size_t)m + j] = jd;
        } else o[(size_t)m + j] = -1;
        U.kept[j] = i;
        src[ex & 0xffff] = (int)threadIdx.x;
    }
    if (U.rows == nullptr) return;                                    // workgroup-uniform
    __syncthreads();
    // the chunk's kept rows, 16 bytes per lane and four lanes to a row: a wave writes 1 KB of consecutive memory
    const int n_kept = total & 0xffff;
    for (int t = (int)threadIdx.x; t < 4 * n_kept; t += kFrChunk) {
        const int r = t >> 2, q = t & 3;
        U.rows_out[4 * (size_t)(base + r) + q] = U.rows[4 * (size_t)(first + src[r]) + q];
    }
}
#else
;
#endif

// one camera of one context of a frame put with its depth
struct FrDepthUnit {
    const float4* pts;                 // the context's cloud on the named side, ring-major
    const int* off;                    // its ring offsets, n_rings + 1 entries
    CamWindow W;                       // the store's translation of this camera and the caller's window
    float4* pstack;                    // scratch: this unit's occlusion stacks, parallel to the cloud (velo_depth_kernels.h) ...
    float4* vstack;
    int* ring_cnt;                     // ... and their heights
    float4* kp_point;                  // scratch, per keypoint: the interpolated point ...
    int* flag;                         // ... and whether there is one
    int* image;                        // 64-byte aligned: ids[n] | has_depth[n] | xy[n][2] | cloud[n_with_depth][3], room for n depth points
    velo_tri_obs* obs;                 // VELO_PUT_OBSERVE: the n records and ids lm_append_kernel reads, else null
    int* obs_ids;
    int n_rings, n;                    // n_rings == 0 for a unit without keypoints: nothing is projected for it
    int chunk0, n_chunks;              // this unit's chunks in the call's count array
    int frame, cam;
};

__global__ void __launch_bounds__(256)
fr_depth_project_kernel(const FrDepthUnit* __restrict__ units)
#if VELO_DEF_FRAMES
{
    const FrDepthUnit& U = units[blockIdx.y];
    const int ring = blockIdx.x;
    if (ring >= U.n_rings) return;                                    // workgroup-uniform
    project_ring(U.pts, U.off, ring, U.W, U.pstack, U.vstack, U.ring_cnt);
}
#else
;
#endif

__global__ void __launch_bounds__(256)
fr_depth_assoc_kernel(const FrDepthUnit* __restrict__ units, double thresh)
#if VELO_DEF_FRAMES
{
    const FrDepthUnit& U = units[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (k >= U.n) return;                                             // wave-uniform
    depth_assoc_keypoint(reinterpret_cast<const float2*>(U.image + 2 * (size_t)U.n), k, lane, U.pstack, U.vstack, U.off, U.ring_cnt, U.n_rings,
                         thresh, U.kp_point, U.flag);
}
#else
;
#endif

__global__ void __launch_bounds__(kFrChunk)
fr_depth_count_kernel(const FrDepthUnit* __restrict__ units, int* __restrict__ counts)
#if VELO_DEF_FRAMES
{
    const FrDepthUnit& U = units[blockIdx.y];
    const int first = blockIdx.x * kFrChunk;
    if (first >= U.n) return;                                         // workgroup-uniform
    const int i = first + (int)threadIdx.x;
    int total;
    (void)block_exclusive_scan(i < U.n ? U.flag[i] : 0, &total);
    if (threadIdx.x == 0) counts[U.chunk0 + blockIdx.x] = total;
}
#else
;
#endif

__global__ void __launch_bounds__(kFrChunk)
fr_depth_write_kernel(const FrDepthUnit* __restrict__ units, const int* __restrict__ counts)
#if VELO_DEF_FRAMES
{
    __shared__ int part[kFrChunk / kWave];
    const FrDepthUnit& U = units[blockIdx.y];
    const int first = blockIdx.x * kFrChunk;
    if (first >= U.n) return;                                         // workgroup-uniform
    int before = 0;                                                   // depth points of the unit's chunks before this one
    for (int k = (int)threadIdx.x; k < (int)blockIdx.x; k += kFrChunk) before += counts[U.chunk0 + k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = before;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < kFrChunk / kWave; w++) base += part[w];
    const int i = first + (int)threadIdx.x;
    const int f = i < U.n ? U.flag[i] : 0;
    int total;
    const int j = base + block_exclusive_scan(f, &total);
    if (i >= U.n) return;
    int* has_depth = U.image + (size_t)U.n;
    if (f != 0) {                                                     // velo.h:481-483: appended in keypoint order
        const float4 p = U.kp_point[i];
        float* q = reinterpret_cast<float*>(U.image + 4 * (size_t)U.n) + 3 * (size_t)j;
        q[0] = p.x; q[1] = p.y; q[2] = p.z;
        has_depth[i] = j;
    } else has_depth[i] = -1;
}
#else
;
#endif

// main.cpp:622-645's choice for entry i of the unit's image: the depth point when it has one (3-D), else the keypoint (2-D)
__global__ void __launch_bounds__(256)
fr_depth_obs_kernel(const FrDepthUnit* __restrict__ units)
#if VELO_DEF_FRAMES
{
    const FrDepthUnit& U = units[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= U.n || U.obs == nullptr) return;
    const int h = U.image[(size_t)U.n + i];
    velo_tri_obs o;
    o.frame = U.frame; o.cam = U.cam;
    if (h == -1) {
        const float* xy = reinterpret_cast<const float*>(U.image + 2 * (size_t)U.n) + 2 * (size_t)i;
        o.kind = VELO_TRI_OBS_2D; o.s[0] = xy[0]; o.s[1] = xy[1]; o.s[2] = 0.0f;
    } else {
        const float* p = reinterpret_cast<const float*>(U.image + 4 * (size_t)U.n) + 3 * (size_t)h;
        o.kind = VELO_TRI_OBS_3D; o.s[0] = p[0]; o.s[1] = p[1]; o.s[2] = p[2];
    }
    U.obs[i] = o;
    U.obs_ids[i] = U.image[i];
}
#else
;
#endif

}  // namespace velo
