// velo_track_kernels.h -- pyramidal Lucas-Kanade tracking: the reference's trackFeatures (velo.h:28-116, cv::calcOpticalFlowPyrLK with a
// 21 x 21 window over 5 levels, kitti.h:5-6).  Defined in velo_unit_track.hip (VELO_DEF_TRACK); gfx950 only.  The arithmetic is that of
// tests/lk_ref.py (OpenCV 3.x lkpyramid.cpp as restated in DESIGN.md 2); the GPU equals it bit for bit.
//
// Resident images (velo_set_images): per camera and slot, every level l of the pyramid is stored padded by kLkPad pixels on every side,
// the image as uint8 (border reflect-101) and the Scharr derivatives as one 32-bit word per pixel (dx in the low, dy in the high 16 bits;
// border zero, BORDER_CONSTANT).  A slot holds all cameras of a call, camera-major, `cam_pix` pixels apart.
//
// Every kernel is table-driven: a call (of one context or of several, possibly of different image sizes) uploads small device tables
// with its input -- one LkBuildUnit per camera of every context, one LkJob per tracking job with the bases of its cameras resolved on
// the host, and the distinct LkPyr level tables both index.  The index is uniform per workgroup (build) or made uniform per wave
// (track: readfirstlane), so the tables are read with scalar loads, once, outside the loops.  The single-context entry points
// (velo_set_images, velo_track_features) are calls with one context: there is no other kernel set.
//
// lk_build_kernel: one launch per level for every camera of every context; the grid is sized for the largest unit, and a unit that has
// no such level or tile leaves at once.  A 16 x 16 tile of padded output pixels; the block first evaluates the level's value at the
// reflect-101 position of every tile pixel and a one-pixel halo into LDS (level 0: the raw upload; level l > 0: pyrDown of the stored
// level l - 1, 25 integer taps), then writes the padded image (border included) and, inside the image, the derivatives from the LDS
// tile -- the halo holds the reflected neighbours, so the border rule of calcSharrDeriv falls out of the indexing.
//
// lk_track_kernel_<N>: ONE WAVE PER POINT, all levels coarse to fine inside the wave.  Lane l owns window pixels l, l + 64, ...: N per
// lane (N = 4 / 8 / 16 for windows up to 15 / 22 / 31).  At each level the lane keeps its share of the resampled I patch and of
// (Ix, Iy) in VGPRs; every iteration samples the lane's J pixels bilinearly, forms diff * Ix and diff * Iy in int32 (|diff| <= 8160,
// |Ix| <= 4080: a lane's sum stays below 2^31) and the wave adds the 64 partial sums in int64 (butterfly: every lane ends with the same
// exact total).  The float steps after the sums are computed redundantly by every lane from identical inputs, so control flow is
// uniform.  Integer sums are exact, hence independent of the reduction order: what lets the result equal the restatement bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef VELO_DEF_TRACK
#define VELO_DEF_TRACK 0
#endif

namespace velo {

constexpr int kLkPad = 32;                 // border of every stored level (>= the largest window)
constexpr int kLkMaxLevel = 7;             // deepest level stored / accepted as max_level
constexpr int kLkLevels = kLkMaxLevel + 1;
constexpr int kLkMinWin = 5, kLkMaxWin = 31;
constexpr int kLkMaxCams = 8;
constexpr int kLkTile = 16;                // build kernel: output tile edge (256 threads)
constexpr int kLkThreads = 256;            // track kernel: 4 waves = 4 points per workgroup
constexpr int kLkWBits = 14;

struct LkLevel {
    int w, h, stride, pad_;                // unpadded size; stride = w + 2 kLkPad (elements per padded row)
    long long off;                         // first element of the padded plane inside one camera's share of the slot
};
struct LkPyr {
    int n_levels, pad_;
    LkLevel lv[kLkLevels];
};

struct LkParams {                          // what every point of a call shares
    int win;
    int max_count;
    float min_eig;
    int pad_;
    double eps2;                           // epsilon^2 (calcOpticalFlowPyrLK squares it)
    double flow_outlier;
};

struct LkBuildUnit {                       // build: one camera of one context
    const unsigned char* raw;              // its w0 x h0 upload
    unsigned char* pix;                    // its share of the context's current slot
    int* der;
    int pyr, pad_;                         // index into the call's table of distinct LkPyr
};

struct LkJob {                             // tracking: one velo_track_job with the bases of its context's cameras resolved
    int first, n;                          // the job's points [first, first + n) of the call
    int pyr, top;                          // level table of its context's image size; deepest level tracked at that size
    const unsigned char* prev_pix;         // previous image of prev_cam (camera base inside the previous slot)
    const int* prev_der;
    const unsigned char* cur_pix;          // current image of cam
};

__device__ __forceinline__ int lk_refl(int i, int n) {       // borderInterpolate(BORDER_REFLECT_101), any offset
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    int q = i % period;
    if (q < 0) q += period;
    return q >= n ? period - q : q;
}

__device__ __forceinline__ int lk_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// level value at (x, y) inside the image (already reflected): the raw upload at level 0, pyrDown of the stored level below otherwise
__device__ __forceinline__ int lk_value(const unsigned char* __restrict__ raw, const unsigned char* __restrict__ below, const LkLevel& B,
                                        int lev, int w0, int x, int y) {
    if (lev == 0) return raw[(size_t)y * w0 + x];
    // taps 2x-2 .. 2x+2 of level l-1 lie within [-2, w_{l-1} + 1]: inside the stored border, which is reflect-101 already
    const unsigned char* p = below + B.off + (long long)(2 * y - 2 + kLkPad) * B.stride + (2 * x - 2 + kLkPad);
    const int k[5] = {1, 4, 6, 4, 1};
    int s = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const unsigned char* r = p + (long long)j * B.stride;
        const int t = r[0] + 4 * r[1] + 6 * r[2] + 4 * r[3] + r[4];
        s += k[j] * t;
    }
    return (s + 128) >> 8;
}

// one 16 x 16 tile of one level of one camera: craw its upload, cpix / cder its share of the slot, L the level, B the level below
__device__ __forceinline__ void lk_build_body(const unsigned char* __restrict__ craw, unsigned char* __restrict__ cpix, int* __restrict__ cder,
                                              const LkLevel L, const LkLevel B, int lev, int w0, int (*tile)[kLkTile + 2]) {
    const int X0 = (int)blockIdx.x * kLkTile - 1, Y0 = (int)blockIdx.y * kLkTile - 1;      // padded coordinates of tile[0][0]
    for (int i = threadIdx.x; i < (kLkTile + 2) * (kLkTile + 2); i += kLkTile * kLkTile) {
        const int ty = i / (kLkTile + 2), tx = i - ty * (kLkTile + 2);
        const int x = lk_refl(X0 + tx - kLkPad, L.w), y = lk_refl(Y0 + ty - kLkPad, L.h);
        tile[ty][tx] = lk_value(craw, cpix, B, lev, w0, x, y);
    }
    __syncthreads();
    const int tx = threadIdx.x % kLkTile, ty = threadIdx.x / kLkTile;
    const int X = X0 + 1 + tx, Y = Y0 + 1 + ty;
    if (X >= L.w + 2 * kLkPad || Y >= L.h + 2 * kLkPad) return;
    const long long o = L.off + (long long)Y * L.stride + X;
    cpix[o] = (unsigned char)tile[ty + 1][tx + 1];
    const int x = X - kLkPad, y = Y - kLkPad;
    int d = 0;
    if (x >= 0 && x < L.w && y >= 0 && y < L.h) {
        int t0[3], t1[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const int a = tile[ty][tx + c], b = tile[ty + 1][tx + c], e = tile[ty + 2][tx + c];
            t0[c] = 3 * (a + e) + 10 * b;
            t1[c] = e - a;
        }
        const int dx = t0[2] - t0[0];
        const int dy = 3 * (t1[2] + t1[0]) + 10 * t1[1];
        d = (int)(((unsigned)dx & 0xFFFFu) | ((unsigned)dy << 16));
    }
    cder[o] = d;
}

// one level of every camera of every context: grid (tiles x, tiles y, units), sized for the largest unit; a unit that has no such level
// or no such tile leaves at once (uniform per workgroup, before any barrier)
__global__ void __launch_bounds__(kLkTile * kLkTile)
lk_build_kernel(const LkBuildUnit* __restrict__ units, const LkPyr* __restrict__ pyrs, int lev)
#if VELO_DEF_TRACK
{
    __shared__ int tile[kLkTile + 2][kLkTile + 2];
    const LkBuildUnit U = units[blockIdx.z];
    const LkPyr* __restrict__ P = pyrs + U.pyr;
    if (lev >= P->n_levels) return;
    const LkLevel L = P->lv[lev];
    if ((int)blockIdx.x * kLkTile >= L.w + 2 * kLkPad || (int)blockIdx.y * kLkTile >= L.h + 2 * kLkPad) return;
    lk_build_body(U.raw, U.pix, U.der, L, P->lv[lev > 0 ? lev - 1 : 0], lev, P->lv[0].w, tile);
}
#else
;
#endif

__device__ __forceinline__ long long lk_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the window's corner (floor of the point) inside [-win, w) x [-win, h)
__device__ __forceinline__ bool lk_in_bounds(float x, float y, int win, int w, int h) {
    return x >= (float)-win && x < (float)w && y >= (float)-win && y < (float)h;
}

__device__ __forceinline__ void lk_weights(float a, float b, int* w00, int* w01, int* w10, int* w11) {
    const float s = (float)(1 << kLkWBits);
    *w00 = __float2int_rn(((1.f - a) * (1.f - b)) * s);
    *w01 = __float2int_rn((a * (1.f - b)) * s);
    *w10 = __float2int_rn(((1.f - a) * b) * s);
    *w11 = (1 << kLkWBits) - *w00 - *w01 - *w10;
}

// the job that owns point i: the last job whose first <= i (empty jobs share their first with the next job)
__device__ __forceinline__ int lk_job_of(const LkJob* __restrict__ jobs, int n_jobs, int i) {
    int lo = 0, hi = n_jobs;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].first <= i) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// diag (diagnostics build only, else null): [level] iterations taken, [kLkLevels + level] points that entered the iteration loop
// point gi of the call: I0 / D0 the previous image and derivatives of its job's prev_cam, J0 the current image of its cam (camera bases),
// P the level table of that image size, top the deepest level tracked
template <int N>
__device__ __forceinline__ void lk_track_point(int gi, const unsigned char* __restrict__ I0, const int* __restrict__ D0,
                                               const unsigned char* __restrict__ J0, const LkPyr& P, int top, const LkParams& A,
                                               const float2* __restrict__ pts, float2* __restrict__ out_xy,
                                               unsigned char* __restrict__ out_status, unsigned char* __restrict__ out_kept,
                                               unsigned long long* __restrict__ diag) {
    const int lane = threadIdx.x & 63;
    const float2 p = pts[gi];
    const int win = A.win, npix = win * win;
    const float hw = (float)(win - 1) * 0.5f;
    int oy[N], ox[N];
#pragma unroll
    for (int k = 0; k < N; k++) {
        const int q = lane + 64 * k;
        oy[k] = q / win;
        ox[k] = q - oy[k] * win;
    }
    bool status = true;
    float sx = 0.f, sy = 0.f;                                  // nextPts[i]
    for (int lev = top; lev >= 0; lev--) {
        const LkLevel L = P.lv[lev];
        const float scale = 1.f / (float)(1 << lev);
        const float px = p.x * scale, py = p.y * scale;
        if (lev == top) { sx = px; sy = py; } else { sx = sx * 2.f; sy = sy * 2.f; }
        const float ppx = px - hw, ppy = py - hw;
        // floor(v) in [-win, n) <=> v in [-win, n) (integer bounds): tested on the float, so NaN fails and no out-of-range value is converted
        if (!lk_in_bounds(ppx, ppy, win, L.w, L.h)) {
            if (lev == 0) status = false;
            continue;
        }
        const int ix = (int)floorf(ppx), iy = (int)floorf(ppy);
        int w00, w01, w10, w11;
        lk_weights(ppx - (float)ix, ppy - (float)iy, &w00, &w01, &w10, &w11);
        const int S = L.stride;
        const long long base = L.off + (long long)(iy + kLkPad) * S + (ix + kLkPad);
        const unsigned char* Ip = I0 + base;
        const int* Dp = D0 + base;
        int Iv[N], Ixv[N], Iyv[N];
        int a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
        for (int k = 0; k < N; k++) {
            Iv[k] = Ixv[k] = Iyv[k] = 0;
            if (lane + 64 * k < npix) {
                const int o = oy[k] * S + ox[k];
                Iv[k] = lk_descale(Ip[o] * w00 + Ip[o + 1] * w01 + Ip[o + S] * w10 + Ip[o + S + 1] * w11, kLkWBits - 5);
                const int d00 = Dp[o], d01 = Dp[o + 1], d10 = Dp[o + S], d11 = Dp[o + S + 1];
                Ixv[k] = lk_descale((int)(short)d00 * w00 + (int)(short)d01 * w01 + (int)(short)d10 * w10 + (int)(short)d11 * w11, kLkWBits);
                Iyv[k] = lk_descale((d00 >> 16) * w00 + (d01 >> 16) * w01 + (d10 >> 16) * w10 + (d11 >> 16) * w11, kLkWBits);
                a11 += Ixv[k] * Ixv[k];
                a12 += Ixv[k] * Iyv[k];
                a22 += Iyv[k] * Iyv[k];
            }
        }
        const float FLT_SCALE = 1.f / (float)(1 << 20);
        const float A11 = (float)lk_wave_sum(a11) * FLT_SCALE;
        const float A12 = (float)lk_wave_sum(a12) * FLT_SCALE;
        const float A22 = (float)lk_wave_sum(a22) * FLT_SCALE;
        const float D = A11 * A22 - A12 * A12;
        const float minEig = (A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12)) / (float)(2 * win * win);
        if (minEig < A.min_eig || D < 1.19209290e-07f) {
            if (lev == 0) status = false;
            continue;
        }
        const float Dinv = 1.f / D;
        float nx = sx - hw, ny = sy - hw;
        float pdx = 0.f, pdy = 0.f;
        int iters = 0;
        for (int j = 0; j < A.max_count; j++) {
            if (!lk_in_bounds(nx, ny, win, L.w, L.h)) {
                if (lev == 0) status = false;
                break;
            }
            const int jx = (int)floorf(nx), jy = (int)floorf(ny);
            iters++;
            lk_weights(nx - (float)jx, ny - (float)jy, &w00, &w01, &w10, &w11);
            const unsigned char* Jp = J0 + L.off + (long long)(jy + kLkPad) * S + (jx + kLkPad);
            int b1 = 0, b2 = 0;
#pragma unroll
            for (int k = 0; k < N; k++) {
                if (lane + 64 * k < npix) {
                    const int o = oy[k] * S + ox[k];
                    const int diff = lk_descale(Jp[o] * w00 + Jp[o + 1] * w01 + Jp[o + S] * w10 + Jp[o + S + 1] * w11, kLkWBits - 5) - Iv[k];
                    b1 += diff * Ixv[k];
                    b2 += diff * Iyv[k];
                }
            }
            const float B1 = (float)lk_wave_sum(b1) * FLT_SCALE;
            const float B2 = (float)lk_wave_sum(b2) * FLT_SCALE;
            const float dx = (A12 * B2 - A22 * B1) * Dinv;
            const float dy = (A12 * B1 - A11 * B2) * Dinv;
            nx = nx + dx;
            ny = ny + dy;
            sx = nx + hw;
            sy = ny + hw;
            if ((double)dx * (double)dx + (double)dy * (double)dy <= A.eps2) break;
            if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
                sx = sx - dx * 0.5f;
                sy = sy - dy * 0.5f;
                break;
            }
            pdx = dx;
            pdy = dy;
        }
        if (diag && lane == 0) {
            atomicAdd(&diag[lev], (unsigned long long)iters);
            atomicAdd(&diag[kLkLevels + lev], 1ull);
        }
    }
    if (lane == 0) {
        out_xy[gi] = make_float2(sx, sy);
        out_status[gi] = status ? 1 : 0;
        // velo.h:72-84: status, util::dist2 (float) against flow_outlier as double, inside [0, width) x [0, height)
        const float ex = p.x - sx, ey = p.y - sy;
        const double d2 = (double)(ex * ex + ey * ey);
        const bool inside = !(sx < 0.f || sy < 0.f || sx >= (float)P.lv[0].w || sy >= (float)P.lv[0].h);
        out_kept[gi] = (status && !(d2 > A.flow_outlier) && inside) ? 1 : 0;
    }
}

template <int N>
__device__ __forceinline__ void lk_track_body(const LkJob* __restrict__ jobs, int n_jobs, const LkPyr* __restrict__ pyrs,
                                              const float2* __restrict__ pts, int total, const LkParams& K, float2* __restrict__ out_xy,
                                              unsigned char* __restrict__ out_status, unsigned char* __restrict__ out_kept,
                                              unsigned long long* __restrict__ diag) {
    // a wave is one point: its index is the same in every lane; saying so keeps the search, the job record and the level table in
    // scalar registers and scalar loads
    const int gi = __builtin_amdgcn_readfirstlane((int)blockIdx.x * (kLkThreads / 64) + (int)(threadIdx.x >> 6));
    if (gi >= total) return;                                   // the whole wave leaves together
    const LkJob J = jobs[lk_job_of(jobs, n_jobs, gi)];
    lk_track_point<N>(gi, J.prev_pix, J.prev_der, J.cur_pix, pyrs[J.pyr], J.top, K, pts, out_xy, out_status, out_kept, diag);
}

#define VELO_LK_TRACK_KERNEL(NAME, N)                                                                                                   \
    __global__ void __launch_bounds__(kLkThreads)                                                                                       \
    NAME(const LkJob* __restrict__ jobs, int n_jobs, const LkPyr* __restrict__ pyrs, const float2* __restrict__ pts, int total,         \
         LkParams K, float2* __restrict__ out_xy, unsigned char* __restrict__ out_status, unsigned char* __restrict__ out_kept,         \
         unsigned long long* __restrict__ diag)
#if VELO_DEF_TRACK
VELO_LK_TRACK_KERNEL(lk_track_kernel_4, 4) { lk_track_body<4>(jobs, n_jobs, pyrs, pts, total, K, out_xy, out_status, out_kept, diag); }
VELO_LK_TRACK_KERNEL(lk_track_kernel_8, 8) { lk_track_body<8>(jobs, n_jobs, pyrs, pts, total, K, out_xy, out_status, out_kept, diag); }
VELO_LK_TRACK_KERNEL(lk_track_kernel_16, 16) { lk_track_body<16>(jobs, n_jobs, pyrs, pts, total, K, out_xy, out_status, out_kept, diag); }
#else
VELO_LK_TRACK_KERNEL(lk_track_kernel_4, 4);
VELO_LK_TRACK_KERNEL(lk_track_kernel_8, 8);
VELO_LK_TRACK_KERNEL(lk_track_kernel_16, 16);
#endif
#undef VELO_LK_TRACK_KERNEL

}  // namespace velo
