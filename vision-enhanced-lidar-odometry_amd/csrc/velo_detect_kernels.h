// velo_detect_kernels.h -- corner detection on the resident images: the reference's detectFeatures (velo.h:118-177), i.e.
// cv::goodFeaturesToTrack(blockSize = 3, minimum eigenvalue) + the occupancy filter against the frame's existing points.  Defined in
// velo_unit_detect.hip (VELO_DEF_DETECT); gfx950 only.  The arithmetic is that of tests/gftt_ref.py; the GPU equals it
// bit for bit.  A call works on UNITS (the distinct cameras its jobs name); every launch covers all units / all jobs.
//
// gf_response_kernel: a 16 x 16 tile of pixels per workgroup.  The padded level-0 image (reflect-101 already) goes to LDS with a 2-pixel
//   halo; the Sobel products dx^2, dx dy, dy^2 of the tile and a 1-pixel halo follow, each evaluated AT THE REFLECTED POSITION of its
//   pixel (the box filter reflects the product maps, not the image: dx changes sign across the border, dx dy with it); the 3 x 3 box
//   sums are int32 and exact, also as float32; the float tail is gftt_ref._tail operation by operation (contraction is off for the
//   whole library).  The tile maximum is merged with a vector atomicMax on the bit pattern (negative values clamp to 0).
// gf_candidates_kernel: threshold, 3 x 3 local-maximum test on the map (v > thr and v >= every neighbour: the same set as "equal to the
//   dilated thresholded map", thr >= 0), a state byte per pixel (0 none, 1 undecided candidate) and the compacted list of candidate
//   pixel indices.  The list order varies from run to run; nothing after it depends on it.
// gf_round_kernel / gf_finish_kernel: the greedy minimum-distance selection as the lexicographically first maximal independent set.  A
//   candidate's key is (value bits, row-major index), larger first.  An undecided candidate is ACCEPTED when every candidate in range
//   with a larger key is dropped, and DROPPED when one of them is accepted; both verdicts are final and depend on larger keys only, so
//   they may be written in place at any time and read by any other thread (no barrier is needed for correctness, only for progress).
//   Neighbours are found in the state map itself, four pixels per 32-bit load; the map is padded by 64 zero pixels so that no load
//   needs a bounds test.  A few launches of gf_round_kernel (one pass over the candidates each, all workgroups) decide the bulk;
//   gf_finish_kernel (one workgroup per unit) then loops over what is still undecided until nothing is -- each pass decides at least
//   the largest undecided key, so it ends, whatever the chain length -- gathers the accepted keys, sorts them (bitonic, descending;
//   in LDS up to 4,096 keys, in global memory above) and applies the cap.
// gf_output_kernel: per job and accepted corner the fresh flag against the job's existing points (LDS chunks, brute force), written in
//   key order; counts per job.
//
// Every kernel works on ONE unit per workgroup through a GfUnit (the unit's image plane, size and its share of every scratch buffer) and
// the call's GfParams.  The GfUnit comes from a device table uploaded with the jobs, at an index that is uniform per workgroup -- scalar
// loads, once; the host resolves the camera bases, so units of several contexts and of different image sizes share the same launches
// (velo_detect_features_batch) and a single-context call (velo_detect_features) is a table of its own cameras: there is no other kernel
// set.  Grids are sized for the largest unit; a workgroup outside its unit's image leaves at once.  The selection stays per unit:
// verdicts depend on that unit's keys and states only, so gf_finish's proof of progress holds for every unit independently.  A unit's
// header is a 128-byte line of its own (kGfHdrStride), so that the per-workgroup atomics of different units do not queue on one line.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "velo_track_kernels.h"

#ifndef VELO_DEF_DETECT
#define VELO_DEF_DETECT 0
#endif

namespace velo {

constexpr int kGfTile = 16;                // response kernel: output tile edge (256 threads)
constexpr int kGfStatePad = 64;            // zero border of the state map (>= the largest min_distance)
constexpr int kGfMaxDist = 64;
constexpr int kGfRoundLaunches = 4;        // passes by the whole device before the single-workgroup loop
constexpr int kGfRoundBlocks = 96;         // workgroups per unit in a pass
constexpr int kGfFinishThreads = 1024;
constexpr int kGfSortLds = 4096;           // keys sorted in LDS (32 KB)
constexpr int kGfOutBlocks = 16;           // workgroups per job in the output kernel
constexpr int kGfHdr = 8;                  // ints per unit: max bits, candidates, accepted, corners (capped), passes, undecided at finish
constexpr int kGfHdrStride = 32;           // ints between the headers of two units: a 128-byte line each

enum { kGfNone = 0, kGfUndecided = 1, kGfAccepted = 2, kGfDropped = 3 };

struct GfJob {
    int unit;                              // index into the call's unit table
    int first, n;                          // the job's existing points [first, first + n) of the call
    int pad_;
};

struct GfUnit {                            // one camera of one context, and its share of the call's scratch
    const unsigned char* plane;            // padded level 0 of the current image (element 0 = padded pixel (0, 0))
    float* eig;                            // h x w
    unsigned char* state;                  // padded state map, rows sstride apart
    unsigned* cand;                        // h x w: candidate pixel indices
    unsigned* und;                         // h x w: undecided at the start of the finish kernel
    unsigned long long* keys;              // a power of two >= h x w
    int* hdr;                              // kGfHdr ints, kGfHdrStride apart from the next unit's
    int w, h, stride, sstride;             // stride: elements per padded image row
};

struct GfParams {                          // what every unit of a call shares
    float scale2;
    int radius;                            // ceil(min_distance) - 1: the largest |dx| in range
    int max_corners;
    int capacity;                          // corners written per job
    double quality, md2;
    float md2f;                            // (float)(min_distance^2), the reference's md2
    int pad_;
};

struct GfResponseLds {
    int img[kGfTile + 4][kGfTile + 4];
    int pxx[kGfTile + 2][kGfTile + 2], pxy[kGfTile + 2][kGfTile + 2], pyy[kGfTile + 2][kGfTile + 2];
    unsigned smax;
};

__device__ __forceinline__ void gf_response_body(const GfUnit& U, const GfParams& A, GfResponseLds& S) {
    auto& img = S.img; auto& pxx = S.pxx; auto& pxy = S.pxy; auto& pyy = S.pyy;
    unsigned& smax = S.smax;
    const int w = U.w, h = U.h;
    const unsigned char* plane = U.plane;
    const int X0 = (int)blockIdx.x * kGfTile, Y0 = (int)blockIdx.y * kGfTile;
    if (threadIdx.x == 0) smax = 0u;
    // x in [X0 - 2, X0 + 18) lies within [-2, w + 16]: inside the 32-pixel border
    for (int i = threadIdx.x; i < (kGfTile + 4) * (kGfTile + 4); i += kGfTile * kGfTile) {
        const int ty = i / (kGfTile + 4), tx = i - ty * (kGfTile + 4);
        img[ty][tx] = plane[(long long)(Y0 - 2 + ty + kLkPad) * U.stride + (X0 - 2 + tx + kLkPad)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (kGfTile + 2) * (kGfTile + 2); i += kGfTile * kGfTile) {
        const int py = i / (kGfTile + 2), px = i - py * (kGfTile + 2);
        const int x = X0 - 1 + px, y = Y0 - 1 + py;
        int xx = 0, xy = 0, yy = 0;
        if (x <= w && y <= h) {
            // the product map's own reflection: -1 -> 1, w -> w - 2, both inside this tile's image patch
            const int lx = lk_refl(x, w) - (X0 - 2), ly = lk_refl(y, h) - (Y0 - 2);
            const int a = img[ly - 1][lx - 1], b = img[ly - 1][lx], c = img[ly - 1][lx + 1];
            const int d = img[ly][lx - 1], f = img[ly][lx + 1];
            const int g = img[ly + 1][lx - 1], k = img[ly + 1][lx], l = img[ly + 1][lx + 1];
            const int dx = (c + 2 * f + l) - (a + 2 * d + g);
            const int dy = (g + 2 * k + l) - (a + 2 * b + c);
            xx = dx * dx; xy = dx * dy; yy = dy * dy;
        }
        pxx[py][px] = xx; pxy[py][px] = xy; pyy[py][px] = yy;
    }
    __syncthreads();
    const int tx = threadIdx.x % kGfTile, ty = threadIdx.x / kGfTile;
    const int x = X0 + tx, y = Y0 + ty;
    if (x < w && y < h) {
        int sxx = 0, sxy = 0, syy = 0;
#pragma unroll
        for (int j = 0; j < 3; j++)
#pragma unroll
            for (int i = 0; i < 3; i++) { sxx += pxx[ty + j][tx + i]; sxy += pxy[ty + j][tx + i]; syy += pyy[ty + j][tx + i]; }
        const float a = ((float)sxx * A.scale2) * 0.5f;
        const float b = (float)sxy * A.scale2;
        const float c = ((float)syy * A.scale2) * 0.5f;
        const float d = a - c;
        const float v = (a + c) - sqrtf(d * d + b * b);
        U.eig[(long long)y * w + x] = v;
        if (v > 0.f) atomicMax(&smax, __float_as_uint(v));
    }
    __syncthreads();
    if (threadIdx.x == 0 && smax != 0u) atomicMax((unsigned*)&U.hdr[0], smax);
}

// grid (tiles x, tiles y, units) for the largest unit
__global__ void __launch_bounds__(kGfTile * kGfTile) gf_response_kernel(const GfUnit* __restrict__ units, GfParams K)
#if VELO_DEF_DETECT
{
    __shared__ GfResponseLds S;
    const GfUnit U = units[blockIdx.z];
    if ((int)blockIdx.x * kGfTile >= U.w || (int)blockIdx.y * kGfTile >= U.h) return;
    gf_response_body(U, K, S);
}
#else
;
#endif

__device__ __forceinline__ unsigned char* gf_state_at(const GfUnit& U, int x, int y) {
    return U.state + (long long)(y + kGfStatePad) * U.sstride + (x + kGfStatePad);
}

// 64 x 4 pixels per workgroup
__device__ __forceinline__ void gf_candidates_body(const GfUnit& U, const GfParams& A, int& s_n, int& s_base) {
    const int w = U.w, h = U.h;
    const float* eig = U.eig;
    const int x = (int)blockIdx.x * 64 + (threadIdx.x & 63), y = (int)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const float maxv = __uint_as_float((unsigned)U.hdr[0]);
    const float thr = (float)((double)maxv * A.quality);
    bool is = false;
    int slot = 0;
    if (x < w && y < h) {
        if (x >= 1 && y >= 1 && x <= w - 2 && y <= h - 2) {
            const float v = eig[(long long)y * w + x];
            if (v > thr) {
                is = true;
#pragma unroll
                for (int j = -1; j <= 1; j++)
#pragma unroll
                    for (int i = -1; i <= 1; i++) is = is && (v >= eig[(long long)(y + j) * w + (x + i)]);
            }
        }
        *gf_state_at(U, x, y) = is ? kGfUndecided : kGfNone;
        if (is) slot = atomicAdd(&s_n, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n > 0) s_base = atomicAdd(&U.hdr[1], s_n);
    __syncthreads();
    if (is) U.cand[s_base + slot] = (unsigned)(y * w + x);
}

// grid (cdiv(w, 64), cdiv(h, 4), units) for the largest unit
__global__ void __launch_bounds__(256) gf_candidates_kernel(const GfUnit* __restrict__ units, GfParams K)
#if VELO_DEF_DETECT
{
    __shared__ int s_n, s_base;
    const GfUnit U = units[blockIdx.z];
    if ((int)blockIdx.x * 64 >= U.w || (int)blockIdx.y * 4 >= U.h) return;
    gf_candidates_body(U, K, s_n, s_base);
}
#else
;
#endif

// the verdict on one undecided candidate from the states around it: kGfAccepted, kGfDropped or still kGfUndecided
__device__ __forceinline__ int gf_decide(const GfUnit& U, const GfParams& A, unsigned idx) {
    const int w = U.w, r = A.radius;
    const int y = (int)(idx / (unsigned)w), x = (int)(idx - (unsigned)y * (unsigned)w);
    const float* eig = U.eig;
    const float v = eig[idx];
    const int w0 = (x + kGfStatePad - r) >> 2, w1 = (x + kGfStatePad + r) >> 2;   // words of a padded row; >= 0, < sstride / 4
    bool blocked = false;
    for (int dy = -r; dy <= r; dy++) {
        const unsigned* row = (const unsigned*)(U.state + (long long)(y + dy + kGfStatePad) * U.sstride);
        for (int wb = w0; wb <= w1; wb += 8) {
            unsigned wv[8];                                    // eight independent loads in flight (a row of the reference's radius is 6-7 words)
#pragma unroll
            for (int q = 0; q < 8; q++) wv[q] = __hip_atomic_load(row + min(wb + q, w1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int wi = wb + q;
                unsigned word = wi <= w1 ? wv[q] : 0u;
                for (int k = 0; word != 0u; k++, word >>= 8) {
                    const unsigned st = word & 0xFFu;
                    if (st == kGfNone || st == kGfDropped) continue;
                    const int nx = (wi << 2) + k - kGfStatePad, ddx = nx - x;
                    const int d2 = ddx * ddx + dy * dy;
                    if (d2 == 0 || !((double)d2 < A.md2)) continue;
                    const unsigned nidx = (unsigned)((y + dy) * w + nx);
                    const float nv = eig[nidx];
                    if (!(nv > v || (nv == v && nidx > idx))) continue;
                    if (st == kGfAccepted) return kGfDropped;
                    blocked = true;
                }
            }
        }
    }
    return blocked ? kGfUndecided : kGfAccepted;
}

__device__ __forceinline__ int gf_load_state(const unsigned char* p) {
    return (int)__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void gf_store_state(unsigned char* p, int s) {
    __hip_atomic_store(p, (unsigned char)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one pass over every candidate of every unit: grid (kGfRoundBlocks, units)
__device__ __forceinline__ void gf_round_body(const GfUnit& U, const GfParams& A) {
    const int n = U.hdr[1];
    const unsigned* cand = U.cand;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const unsigned idx = cand[i];
        unsigned char* sp = gf_state_at(U, (int)(idx % (unsigned)U.w), (int)(idx / (unsigned)U.w));
        if (gf_load_state(sp) != kGfUndecided) continue;
        const int s = gf_decide(U, A, idx);
        if (s != kGfUndecided) gf_store_state(sp, s);
    }
}

__global__ void __launch_bounds__(256) gf_round_kernel(const GfUnit* __restrict__ units, GfParams K)
#if VELO_DEF_DETECT
{
    const GfUnit U = units[blockIdx.y];
    gf_round_body(U, K);
}
#else
;
#endif

// one workgroup per unit: the rest of the selection, the sort of the accepted keys and the cap
struct GfFinishLds {
    unsigned long long skeys[kGfSortLds];
    int s_n, s_left, s_acc;
};

__device__ __forceinline__ void gf_finish_body(const GfUnit& U, const GfParams& A, GfFinishLds& S) {
    auto& skeys = S.skeys;
    int& s_n = S.s_n; int& s_left = S.s_left; int& s_acc = S.s_acc;
    const int tid = threadIdx.x;
    const int w = U.w;
    const int n = U.hdr[1];
    const unsigned* cand = U.cand;
    unsigned* und = U.und;
    const float* eig = U.eig;
    if (tid == 0) { s_n = 0; s_acc = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += kGfFinishThreads) {
        const unsigned idx = cand[i];
        if (gf_load_state(gf_state_at(U, (int)(idx % (unsigned)w), (int)(idx / (unsigned)w))) == kGfUndecided) und[atomicAdd(&s_n, 1)] = idx;
    }
    __syncthreads();
    const int n_und = s_n;
    int passes = kGfRoundLaunches;
    for (int left = n_und; left > 0;) {
        if (tid == 0) s_left = 0;
        __syncthreads();
        for (int i = tid; i < n_und; i += kGfFinishThreads) {
            const unsigned idx = und[i];
            unsigned char* sp = gf_state_at(U, (int)(idx % (unsigned)w), (int)(idx / (unsigned)w));
            if (gf_load_state(sp) != kGfUndecided) continue;
            const int s = gf_decide(U, A, idx);
            if (s != kGfUndecided) gf_store_state(sp, s);
            else atomicAdd(&s_left, 1);
        }
        __threadfence();
        __syncthreads();
        left = s_left;
        passes++;
        __syncthreads();
    }
    // the accepted keys, in any order
    unsigned long long* gkeys = U.keys;
    for (int i = tid; i < n; i += kGfFinishThreads) {
        const unsigned idx = cand[i];
        if (gf_load_state(gf_state_at(U, (int)(idx % (unsigned)w), (int)(idx / (unsigned)w))) == kGfAccepted)
            gkeys[atomicAdd(&s_acc, 1)] = ((unsigned long long)__float_as_uint(eig[idx]) << 32) | idx;
    }
    __syncthreads();
    const int n_acc = s_acc;
    int n2 = 1;
    while (n2 < n_acc) n2 <<= 1;                       // <= keys_cap
    for (int i = n_acc + tid; i < n2; i += kGfFinishThreads) gkeys[i] = 0ull;      // below every key (a candidate's value is > 0)
    __syncthreads();
    const bool in_lds = n2 <= kGfSortLds;
    unsigned long long* a = gkeys;
    if (in_lds) {
        for (int i = tid; i < n2; i += kGfFinishThreads) skeys[i] = gkeys[i];
        a = skeys;
        __syncthreads();
    }
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < n2; i += kGfFinishThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long p = a[i], q = a[l];
                    const bool desc = (i & k) == 0;
                    if (desc ? (p < q) : (p > q)) { a[i] = q; a[l] = p; }
                }
            }
            __syncthreads();
        }
    if (in_lds) for (int i = tid; i < n_acc; i += kGfFinishThreads) gkeys[i] = skeys[i];
    if (tid == 0) {
        U.hdr[2] = n_acc;
        U.hdr[3] = (A.max_corners > 0 && n_acc > A.max_corners) ? A.max_corners : n_acc;
        U.hdr[4] = passes;
        U.hdr[5] = n_und;
    }
}

__global__ void __launch_bounds__(kGfFinishThreads) gf_finish_kernel(const GfUnit* __restrict__ units, GfParams K)
#if VELO_DEF_DETECT
{
    __shared__ GfFinishLds S;
    const GfUnit U = units[blockIdx.x];
    gf_finish_body(U, K, S);
}
#else
;
#endif

// grid (kGfOutBlocks, jobs): xy / response / fresh of the first `capacity` corners in key order; counts [job][3] = corners, fresh, candidates
__device__ __forceinline__ void gf_output_body(const GfUnit& U, const GfParams& A, const GfJob J, const float2* __restrict__ existing,
                                               int* __restrict__ counts, float2* __restrict__ out_xy, float* __restrict__ out_resp,
                                               unsigned char* __restrict__ out_fresh, float2* pts, int& s_fresh) {
    const int j = blockIdx.y;
    const int n_out = U.hdr[3];
    const unsigned long long* keys = U.keys;
    const float fw = (float)U.w, fh = (float)U.h;
    const float md2 = A.md2f;                  // util::dist2 is a float converted to double: (double)d2 < (double)md2f <=> d2 < md2f
    if (threadIdx.x == 0) s_fresh = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { counts[3 * j + 0] = n_out; counts[3 * j + 2] = U.hdr[1]; }
    for (int base = blockIdx.x * 256; base < n_out; base += gridDim.x * 256) {       // uniform per workgroup
        const int i = base + threadIdx.x;
        unsigned long long key = 0ull;
        float cx = 0.f, cy = 0.f;
        if (i < n_out) {
            key = keys[i];
            const unsigned idx = (unsigned)(key & 0xFFFFFFFFull);
            const unsigned y = idx / (unsigned)U.w;
            cx = (float)(idx - y * (unsigned)U.w); cy = (float)y;
        }
        bool bad = false;
        for (int e0 = 0; e0 < J.n; e0 += 256) {
            __syncthreads();
            const int m = min(256, J.n - e0);
            if ((int)threadIdx.x < m) {
                float2 p = existing[J.first + e0 + threadIdx.x];
                // points outside the image or non-finite take no part (NaN fails every comparison)
                if (!(p.x >= 0.f && p.y >= 0.f && p.x < fw && p.y < fh)) p = make_float2(-1.0e9f, -1.0e9f);
                pts[threadIdx.x] = p;
            }
            __syncthreads();
#pragma unroll 8
            for (int e = 0; e < m; e++) {                         // no short circuit: the LDS reads of an unrolled group overlap
                const float dx = pts[e].x - cx, dy = pts[e].y - cy;
                const float d2 = dx * dx + dy * dy;              // util::dist2: float arithmetic
                bad |= (d2 < md2);
            }
        }
        if (i < n_out) {
            if (!bad) atomicAdd(&s_fresh, 1);
            if (i < A.capacity) {
                const long long o = (long long)j * A.capacity + i;
                out_xy[o] = make_float2(cx, cy);
                out_resp[o] = __uint_as_float((unsigned)(key >> 32));
                out_fresh[o] = bad ? 0 : 1;
            }
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_fresh > 0) atomicAdd(&counts[3 * j + 1], s_fresh);
}

__global__ void __launch_bounds__(256) gf_output_kernel(const GfUnit* __restrict__ units, GfParams K, const GfJob* __restrict__ jobs,
                                                        const float2* __restrict__ existing, int* __restrict__ counts,
                                                        float2* __restrict__ out_xy, float* __restrict__ out_resp,
                                                        unsigned char* __restrict__ out_fresh)
#if VELO_DEF_DETECT
{
    __shared__ float2 pts[256];
    __shared__ int s_fresh;
    const GfJob J = jobs[blockIdx.y];
    const GfUnit U = units[J.unit];
    gf_output_body(U, K, J, existing, counts, out_xy, out_resp, out_fresh, pts, s_fresh);
}
#else
;
#endif

}  // namespace velo
