// velo_landmark_kernels.h -- the device-resident landmark store (reference main.cpp:614-679, getLandmarksAtFrame velo.h:1132-1160).
// Included by velo_hip.hip (declarations) and by velo_unit_landmarks.hip (VELO_DEF_LANDMARKS: the definitions); gfx950 only.
//
// What a context keeps on the device (velo_api_landmarks.inl owns the buffers):
//     log[k]   one observation per entry, in arrival order: {kind, frame, cam, s} -- a 3-D entry of keypoint_obs3[id][cam][frame]
//              or a 2-D entry of keypoint_obs2[id][cam][frame]
//     prev[k]  the log index of the previous observation of the SAME landmark (-1: none); head[id] the newest one.  Indices, not
//              pointers: the chains survive a reallocation of the log
//     count[id], added[id], pts[id]   keypoint_obs_count, keypoint_added, landmarks
//     frames[f]  the Rodrigues constants of ceres_poses_vec[f] (TriFrame, velo_tri_kernels.h)
// Triangulating a frame is two launches for all contexts of a call: lm_gather_kernel writes every landmark's observations in the
// reference's block order (3-D first, then 2-D; each camera-major, frame ascending: the iteration order of the per-camera std::map)
// and lm_solve_kernel runs the wave-per-landmark body of velo_tri_kernels.h on them.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/velo_hip.h"
#include "velo_scan_types.h"
#include "velo_tri_kernels.h"

#ifndef VELO_DEF_LANDMARKS
#define VELO_DEF_LANDMARKS 0
#endif

namespace velo {

// one context of a call: where its store lives and how it solves.  Read at a workgroup-uniform index.
struct LmUnit {
    const TriFrame* frames;
    const double* cam_t;
    const velo_tri_obs* log;
    const int* prev;
    const int* head;
    float* pts;
    unsigned char* added;
    TriParams P;
};

struct LmItem { int id, unit; };       // one landmark of a call

struct LmPose { double m[16]; };       // row-major 4 x 4

// block order of an observation inside its landmark: kind (3-D = 0 first), camera, frame
__device__ __forceinline__ unsigned long long lm_order_key(const velo_tri_obs& o) {
    return ((unsigned long long)(unsigned)o.kind << 48) | ((unsigned long long)(unsigned)o.cam << 32) | (unsigned long long)(unsigned)o.frame;
}

// the loop body of main.cpp:622-645 for the n entries of one (frame, camera): entry i becomes log[base + i].  The ids of a call are
// distinct (checked on the host), so no two threads touch the same landmark.
__global__ void __launch_bounds__(256)
lm_append_kernel(const velo_tri_obs* __restrict__ in_obs, const int* __restrict__ in_ids, int n, int base, velo_tri_obs* __restrict__ log,
                 int* __restrict__ prev, int* __restrict__ head, int* __restrict__ count)
#if VELO_DEF_LANDMARKS
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = in_ids[i];
    log[base + i] = in_obs[i];
    prev[base + i] = head[id];
    head[id] = base + i;
    count[id] = count[id] + 1;
}
#else
;
#endif

// One wave per landmark.  Landmark l of the call owns out[off[l] .. off[l + 1]); its chain holds exactly that many entries (the
// host counts what it appends).  Lane j takes the chain positions j, j + 64, ...; the rank of an entry is the number of entries of
// the chain that come before it in block order (the keys of one landmark are distinct: one entry per frame and camera).
__global__ void __launch_bounds__(64)
lm_gather_kernel(const LmUnit* __restrict__ units, const LmItem* __restrict__ items, const int* __restrict__ off, int n, velo_tri_obs* __restrict__ out)
#if VELO_DEF_LANDMARKS
{
    const int l = blockIdx.x;
    if (l >= n) return;
    const LmItem it = items[l];
    const LmUnit& U = units[it.unit];
    const int b = off[l], cnt = off[l + 1] - b;
    const int lane = threadIdx.x;
    const int first = U.head[it.id];
    int cur = first;                                                  // chain position `base`
    for (int base = 0; base < cnt; base += 64) {
        int mine = -1, p = cur;
        for (int k = 0; k < 64 && base + k < cnt && p >= 0; k++) {
            if (k == lane) mine = p;
            p = U.prev[p];
        }
        cur = p;
        if (mine >= 0) {
            const velo_tri_obs o = U.log[mine];
            const unsigned long long key = lm_order_key(o);
            int rank = 0, q = first;
            for (int k = 0; k < cnt && q >= 0; k++) {
                rank += lm_order_key(U.log[q]) < key ? 1 : 0;
                q = U.prev[q];
            }
            if (rank < cnt) out[b + rank] = o;
        }
    }
}
#else
;
#endif

// triangulatePoint for every landmark of the call (main.cpp:661-671): start from the stored point when the landmark was added
// before, else from (0, 0, 10); afterwards the point is stored as float and the landmark is marked added.
__global__ void __launch_bounds__(64)
lm_solve_kernel(const LmUnit* __restrict__ units, const LmItem* __restrict__ items, const velo_tri_obs* __restrict__ obs, const int* __restrict__ off,
                int n, float* __restrict__ out_pts, velo_tri_result* __restrict__ results)
#if VELO_DEF_LANDMARKS
{
    __shared__ TriShared sh;
    const int l = blockIdx.x;
    if (l >= n) return;
    const int lane = threadIdx.x;
    const LmItem it = items[l];
    const LmUnit& U = units[it.unit];
    const TriParams P = U.P;
    const int b = off[l], n_obs = off[l + 1] - b;
    float* pt = U.pts + 3 * (size_t)it.id;
    const bool guess = U.added[it.id] != 0;
    double x[3] = {0.0, 0.0, 10.0};                                   // velo.h:1043
    if (guess) { x[0] = pt[0]; x[1] = pt[1]; x[2] = pt[2]; }         // velo.h:1044-1049
    velo_tri_result S;
    VELO_TRI_WAVE_LANDMARK(U.frames, U.cam_t, obs, b, n_obs, guess, P, x, S)
    if (lane == 0) {
        const float fx = (float)x[0], fy = (float)x[1], fz = (float)x[2];                            // velo.h:1124-1126
        pt[0] = fx; pt[1] = fy; pt[2] = fz;
        U.added[it.id] = 1;                                           // main.cpp:672-678
        out_pts[3 * (size_t)l] = fx; out_pts[3 * (size_t)l + 1] = fy; out_pts[3 * (size_t)l + 2] = fz;
        results[l] = S;
    }
}
#else
;
#endif

// getLandmarksAtFrame (velo.h:1146-1153) for one added landmark: p = M (x, y, z, 1) in double, every row summed left to right,
// divided by p[3] and rounded to float.  Shared with the match assembly (velo_frame_kernels.h), whose landmark points must have
// the bits velo_landmarks_at_frame gives.
__device__ __forceinline__ void lm_move_point(const float* __restrict__ pt, const double* __restrict__ m, float* __restrict__ out) {
    const double q0 = (double)pt[0], q1 = (double)pt[1], q2 = (double)pt[2];
    double p[4];
#pragma unroll
    for (int r = 0; r < 4; r++) p[r] = ((m[4 * r] * q0 + m[4 * r + 1] * q1) + m[4 * r + 2] * q2) + m[4 * r + 3] * 1.0;
    out[0] = (float)(p[0] / p[3]);
    out[1] = (float)(p[1] / p[3]);
    out[2] = (float)(p[2] / p[3]);
}

// ... for n added landmarks
__global__ void __launch_bounds__(256)
lm_at_frame_kernel(const int* __restrict__ ids, int n, const float* __restrict__ pts, LmPose M, float* __restrict__ out)
#if VELO_DEF_LANDMARKS
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    lm_move_point(pts + 3 * (size_t)ids[i], M.m, out + 3 * (size_t)i);
}
#else
;
#endif

// read-back of landmarks, keypoint_added and keypoint_obs_count for n ids; an id the store has never grown to reads as empty
__global__ void __launch_bounds__(256)
lm_get_kernel(const int* __restrict__ ids, int n, int n_ids, const float* __restrict__ pts, const unsigned char* __restrict__ added,
              const int* __restrict__ count, float* __restrict__ out_xyz, int* __restrict__ out_count, unsigned char* __restrict__ out_added)
#if VELO_DEF_LANDMARKS
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int id = ids[i];
    const bool ok = id >= 0 && id < n_ids;
    out_xyz[3 * (size_t)i] = ok ? pts[3 * (size_t)id] : 0.0f;
    out_xyz[3 * (size_t)i + 1] = ok ? pts[3 * (size_t)id + 1] : 0.0f;
    out_xyz[3 * (size_t)i + 2] = ok ? pts[3 * (size_t)id + 2] : 0.0f;
    out_count[i] = ok ? count[id] : 0;
    out_added[i] = ok ? added[id] : (unsigned char)0;
}
#else
;
#endif

}  // namespace velo
