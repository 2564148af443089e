// velo_match_kernels.h -- batched brute-force Hamming matching of 512-bit (FREAK, 64-byte) descriptors: the reference's matchFeatures
// (velo.h:499-549, cv::BFMatcher(NORM_HAMMING).match + the min-distance filter).  Defined in velo_unit_match.hip (VELO_DEF_MATCH);
// gfx950 only.
//
// A batch is n_jobs independent (query set, train set) pairs.  Every descriptor row is 64 bytes; the host stages the DISTINCT sets of a
// call once (a shared query set serves every candidate of a loop-closure batch) and each job names its rows by offset.
//
// Product kernel (match_mfma_kernel): the int8 matrix cores on +-1 bits.  Bit b maps to the int8 1 - 2b, so for two rows
//     <q', t'> = sum (1 - 2 q_k)(1 - 2 t_k) = 512 - 2 popcount(q ^ t),   hamming(q, t) = (512 - <q', t'>) / 2   (exact in int32).
// v_mfma_i32_16x16x64_i8 computes a 16 x 16 block of these dot products over 64 bits per step, 8 steps per descriptor.  The 64-byte
// rows are read as they are (lane l reads the 16 bytes 16 (l >> 4) .. of row l & 15: one coalesced 1 KB load per 16 rows) and expanded
// to +-1 bytes in registers, 4 bits per dword.  The order in which the 512 bits meet the k index is a permutation the two operands
// share (both are loaded by the same lane pattern), and a dot product does not depend on it.
//   A = 16 train rows (expanded per tile), B = 16 queries (expanded once per wave, 4 tiles = 64 queries held in registers).
//   D row 4 (l >> 4) + i = train row, D column l & 15 = query (the C/D map every gfx950 MFMA shape shares; the test suite holds the
//   whole product to a numpy brute force with asymmetric data),
//   so each lane keeps a running minimum per query tile in its own registers and the 4 lane groups meet once at the end.
// Key of a pair = (distance << kMatchIdxBits) | trainIdx: the minimum key is the nearest row with the LOWEST index on ties, like
// cv::BFMatcher's strict `<` scan (velo.h:527-531; the CUDA branch leaves ties unpinned).  Blocks split the query AND the
// train dimension; they merge with vector atomicMin into one key per query and one min_dist per job -- integer minima, so the result
// does not depend on the grid.
//
// Diagnostics-build variant (match_valu_kernel, VELO_MATCH_VARIANT=0 in libvelo_hip_diag.so only): one query per lane, XOR + popcount
// over 8 x u64 against train rows staged in LDS.  Same keys, same result bit for bit (tests/test_gpu_match.py).
//
// Resident rows (match_mfma_resident_kernel, match_filter_resident_kernel): the same two bodies for jobs whose rows already live on
// the device, in the row arenas of one or several contexts' frame stores (velo_api_frames.inl) -- a job names each side by its base
// pointer, nothing is staged.  The product kernel only: the diagnostics variant is not wired to them.
//
// match_filter_kernel: one workgroup per job applies velo.h:536-549 -- keep iff distance <= max(1.5 min_dist, match_thresh), in double
// like the reference -- and writes the kept (queryIdx, trainIdx) pairs in query order with a workgroup exclusive scan.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#ifndef VELO_DEF_MATCH
#define VELO_DEF_MATCH 0
#endif

namespace velo {

constexpr int kMatchIdxBits = 22;                              // key = distance (10 bits, <= 512) << 22 | trainIdx
constexpr int kMatchMaxRows = 1 << kMatchIdxBits;              // train rows per job the key can index
constexpr unsigned kMatchIdxMask = (1u << kMatchIdxBits) - 1u;
constexpr unsigned kMatchNone = 0xFFFFFFFFu;                   // "no pair yet" (every real key is smaller)
constexpr int kMatchThreads = 256;                             // 4 waves
constexpr int kMatchQ = 64;                                    // product kernel: queries per block (4 MFMA tiles of 16)
constexpr int kMatchT = 512;                                   // product kernel: train rows per block (the 4 waves take every 4th tile of 16)
constexpr int kMatchValuQ = 256;                               // variant: queries per block (one per lane)
constexpr int kMatchValuT = 256;                               // variant: train rows per block, staged in LDS (16 KB)

struct MatchJob {        // one (query, train) pair of a call, as the kernels see it
    int q_row, t_row;    // first row of the query / train set in the staged rows (64 bytes each)
    int n_query, n_train;
    int q_out;           // first entry of this job in the per-query outputs (exclusive scan of n_query)
    int blk_start;       // first block of this job in the product / variant grid (exclusive scan of its blocks)
    int nqb;             // query blocks of this job (the grid of a job is nqb x train blocks, query block fastest)
    int pad;
};

struct MatchResJob {     // one (query, train) pair on resident rows: every member but the two pointers means what it means in MatchJob
    const uint4* q;      // first row of the query / train set (64 bytes each, 64-byte aligned), in whatever arena holds it
    const uint4* t;
    int n_query, n_train;
    int q_out;
    int blk_start;
    int nqb;
    int pad;
};

// the job that owns block b: the last job whose blk_start <= b (jobs without blocks share their start with the next job)
template <typename Job>
__device__ __forceinline__ int match_job_of_block(const Job* __restrict__ jobs, int n_jobs, int b) {
    int lo = 0, hi = n_jobs;                 // first job with blk_start > b
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (jobs[mid].blk_start <= b) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

typedef int match_v4i __attribute__((ext_vector_type(4)));

// 4 bits -> 4 int8 of +1 / -1 (bit i -> byte i = 1 - 2 bit): the multiply spreads bit i to bit 8i (x, x << 7, x << 14, x << 21 do not
// overlap for x < 16), then 0xFE * spread + 0x01010101 gives 0x01 or 0xFF per byte without carries
__device__ __forceinline__ int match_pm1_nibble(unsigned x) {
    const unsigned spread = (x * 0x00204081u) & 0x01010101u;
    return (int)(spread * 0xFEu + 0x01010101u);
}

// 16 bits (bits 16 s .. 16 s + 15 of the lane's 128-bit chunk) -> one i8 MFMA operand fragment
__device__ __forceinline__ match_v4i match_expand(const uint4& c, int s) {
    const unsigned w = (s >> 1) == 0 ? c.x : (s >> 1) == 1 ? c.y : (s >> 1) == 2 ? c.z : c.w;
    const unsigned h = (s & 1) ? (w >> 16) : (w & 0xFFFFu);
    match_v4i v;
    v.x = match_pm1_nibble(h & 15u);
    v.y = match_pm1_nibble((h >> 4) & 15u);
    v.z = match_pm1_nibble((h >> 8) & 15u);
    v.w = match_pm1_nibble(h >> 12);
    return v;
}

__device__ __forceinline__ unsigned match_wave_min(unsigned v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, (unsigned)__shfl_xor((int)v, o));
    return v;
}

// ---- product: int8 MFMA on +-1 bits ----------------------------------------------------------------------------------------------
// One block of job j: 64 queries from q0 against the train rows [t_begin, t_begin + kMatchT).  q_rows / t_rows: the job's first query /
// train row; key_out: the job's first key.  The arithmetic of both product kernels.
__device__ __forceinline__ void match_mfma_block(const uint4* __restrict__ q_rows, const uint4* __restrict__ t_rows, int n_query, int n_train,
                                                 int q0, int t_begin, unsigned* __restrict__ key_out, unsigned* __restrict__ job_min) {
    __shared__ unsigned red[kMatchThreads / 64][kMatchQ];
    const int t_end = min(t_begin + kMatchT, n_train);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;

    match_v4i B[4][8];                                      // the block's 64 queries, +-1 bytes (128 VGPRs)
#pragma unroll
    for (int qt = 0; qt < 4; qt++) {
        const int q = min(q0 + qt * 16 + r, n_query - 1);     // rows past the set repeat the last one; their columns are never stored
        const uint4 c = q_rows[(size_t)q * 4 + g];
#pragma unroll
        for (int s = 0; s < 8; s++) B[qt][s] = match_expand(c, s);
    }
    unsigned best[4] = {kMatchNone, kMatchNone, kMatchNone, kMatchNone};   // query q0 + 16 qt + (lane & 15): min key over this lane's train rows
    for (int t = t_begin + wave * 16; t < t_end; t += 16 * (kMatchThreads / 64)) {
        const uint4 c = t_rows[(size_t)min(t + r, n_train - 1) * 4 + g];
        match_v4i acc[4];
#pragma unroll
        for (int qt = 0; qt < 4; qt++) acc[qt] = match_v4i{0, 0, 0, 0};
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const match_v4i a = match_expand(c, s);
#pragma unroll
            for (int qt = 0; qt < 4; qt++) acc[qt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, B[qt][s], acc[qt], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int tt = t + 4 * g + i;                       // D row 4 (lane >> 4) + i
            if (tt < t_end) {
#pragma unroll
                for (int qt = 0; qt < 4; qt++) {
                    const unsigned d = (unsigned)(512 - acc[qt][i]) >> 1;
                    best[qt] = min(best[qt], (d << kMatchIdxBits) | (unsigned)tt);
                }
            }
        }
    }
#pragma unroll
    for (int qt = 0; qt < 4; qt++) {                            // the 4 lane groups hold the same 16 queries
        unsigned v = min(best[qt], (unsigned)__shfl_xor((int)best[qt], 16));
        v = min(v, (unsigned)__shfl_xor((int)v, 32));
        if (g == 0) red[wave][qt * 16 + r] = v;
    }
    __syncthreads();
    if (wave == 0) {
        unsigned v = red[0][lane];
#pragma unroll
        for (int w = 1; w < kMatchThreads / 64; w++) v = min(v, red[w][lane]);
        const int q = q0 + lane;
        if (q >= n_query) v = kMatchNone;
        if (v != kMatchNone) atomicMin(&key_out[q], v);
        const unsigned m = match_wave_min(v);
        if (lane == 0 && m != kMatchNone) atomicMin(job_min, m >> kMatchIdxBits);
    }
}

// rows: the staged descriptor rows as uint4 (4 per row); keys [sum n_query] and min_dist [n_jobs] start at kMatchNone
__global__ void __launch_bounds__(kMatchThreads)
match_mfma_kernel(const uint4* __restrict__ rows, const MatchJob* __restrict__ jobs, int n_jobs, unsigned* __restrict__ keys,
                  unsigned* __restrict__ min_dist)
#if VELO_DEF_MATCH
{
    const int j = match_job_of_block(jobs, n_jobs, (int)blockIdx.x);
    const MatchJob J = jobs[j];
    const int local = (int)blockIdx.x - J.blk_start;
    match_mfma_block(rows + (size_t)J.q_row * 4, rows + (size_t)J.t_row * 4, J.n_query, J.n_train, (local % J.nqb) * kMatchQ,
                     (local / J.nqb) * kMatchT, keys + J.q_out, min_dist + j);
}
#else
;
#endif

// the same on resident rows: every job brings its own two base pointers (a batch names several contexts' arenas)
__global__ void __launch_bounds__(kMatchThreads)
match_mfma_resident_kernel(const MatchResJob* __restrict__ jobs, int n_jobs, unsigned* __restrict__ keys, unsigned* __restrict__ min_dist)
#if VELO_DEF_MATCH
{
    const int j = match_job_of_block(jobs, n_jobs, (int)blockIdx.x);
    const MatchResJob J = jobs[j];
    const int local = (int)blockIdx.x - J.blk_start;
    match_mfma_block(J.q, J.t, J.n_query, J.n_train, (local % J.nqb) * kMatchQ, (local / J.nqb) * kMatchT, keys + J.q_out, min_dist + j);
}
#else
;
#endif

// ---- variant (diagnostics build): XOR + popcount, one query per lane ------------------------------------------------------------
__global__ void __launch_bounds__(kMatchThreads)
match_valu_kernel(const uint4* __restrict__ rows, const MatchJob* __restrict__ jobs, int n_jobs, unsigned* __restrict__ keys,
                  unsigned* __restrict__ min_dist)
#if VELO_DEF_MATCH
{
    __shared__ uint4 tr[kMatchValuT * 4];
    const int j = match_job_of_block(jobs, n_jobs, (int)blockIdx.x);
    const MatchJob J = jobs[j];
    const int local = (int)blockIdx.x - J.blk_start;
    const int q0 = (local % J.nqb) * kMatchValuQ;
    const int t_begin = (local / J.nqb) * kMatchValuT;
    const int cnt = min(kMatchValuT, J.n_train - t_begin);
    for (int i = threadIdx.x; i < cnt * 4; i += kMatchThreads) tr[i] = rows[((size_t)J.t_row + t_begin) * 4 + i];
    const int q = q0 + (int)threadIdx.x;
    const uint4* qp = rows + ((size_t)J.q_row + min(q, J.n_query - 1)) * 4;
    uint64_t qv[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint4 c = qp[k];
        qv[2 * k] = ((uint64_t)c.y << 32) | c.x;
        qv[2 * k + 1] = ((uint64_t)c.w << 32) | c.z;
    }
    __syncthreads();
    unsigned best = kMatchNone;
    for (int t = 0; t < cnt; t++) {                               // every lane reads the same row: an LDS broadcast
        unsigned d = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint4 c = tr[t * 4 + k];
            d += (unsigned)__popcll(qv[2 * k] ^ (((uint64_t)c.y << 32) | c.x));
            d += (unsigned)__popcll(qv[2 * k + 1] ^ (((uint64_t)c.w << 32) | c.z));
        }
        best = min(best, (d << kMatchIdxBits) | (unsigned)(t_begin + t));   // t ascending: strict improvement keeps the lowest index
    }
    if (q >= J.n_query) best = kMatchNone;
    if (best != kMatchNone) atomicMin(&keys[J.q_out + q], best);
    const unsigned m = match_wave_min(best);
    if ((threadIdx.x & 63) == 0 && m != kMatchNone) atomicMin(&min_dist[j], m >> kMatchIdxBits);
}
#else
;
#endif

// ---- velo.h:536-549: threshold and compaction, one workgroup per job ------------------------------------------------------------
// out: idx [sum n_query] | dist [sum n_query] | pairs [sum n_query][2] (job j's kept pairs from entry q_out) | per job {min_dist, n_kept}
__device__ __forceinline__ void match_filter_job(int j, int n_query, int n_train, int q_out, const unsigned* __restrict__ keys,
                                                 const unsigned* __restrict__ min_dist, double match_thresh, int total_q, int* __restrict__ out) {
    __shared__ int wsum[kMatchThreads / 64];
    int* o_idx = out;
    int* o_dist = out + total_q;
    int* o_pairs = out + 2 * (size_t)total_q;
    int* o_job = out + 4 * (size_t)total_q;
    const bool any = n_train > 0 && n_query > 0;
    const unsigned md = any ? min_dist[j] : 0u;
    const double thr = fmax(1.5 * (double)md, match_thresh);     // std::max(1.5*min_dist, match_thresh), velo.h:546
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int c0 = 0; c0 < n_query; c0 += kMatchThreads) {
        const int q = c0 + (int)threadIdx.x;
        bool keep = false;
        int t = -1;
        if (q < n_query) {
            int d = -1;
            if (any) {
                const unsigned k = keys[q_out + q];
                t = (int)(k & kMatchIdxMask);
                d = (int)(k >> kMatchIdxBits);
                keep = !((double)d > thr);                          // velo.h:546: `continue` when distance > max(...)
            }
            o_idx[q_out + q] = t;
            o_dist[q_out + q] = d;
        }
        const uint64_t bal = __ballot(keep);
        const int rank = (int)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wsum[wave] = (int)__popcll(bal);
        __syncthreads();
        int pre = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < kMatchThreads / 64; w++) { const int s = wsum[w]; if (w < wave) pre += s; tot += s; }
        if (keep) {
            const size_t e = (size_t)q_out + base + pre + rank;
            o_pairs[2 * e] = q;
            o_pairs[2 * e + 1] = t;
        }
        base += tot;
        __syncthreads();                                            // wsum is rewritten by the next chunk
    }
    if (threadIdx.x == 0) {
        o_job[2 * j] = any ? (int)md : -1;
        o_job[2 * j + 1] = base;
    }
}

__global__ void __launch_bounds__(kMatchThreads)
match_filter_kernel(const MatchJob* __restrict__ jobs, const unsigned* __restrict__ keys, const unsigned* __restrict__ min_dist,
                    double match_thresh, int total_q, int* __restrict__ out)
#if VELO_DEF_MATCH
{
    const MatchJob J = jobs[blockIdx.x];
    match_filter_job((int)blockIdx.x, J.n_query, J.n_train, J.q_out, keys, min_dist, match_thresh, total_q, out);
}
#else
;
#endif

__global__ void __launch_bounds__(kMatchThreads)
match_filter_resident_kernel(const MatchResJob* __restrict__ jobs, const unsigned* __restrict__ keys, const unsigned* __restrict__ min_dist,
                             double match_thresh, int total_q, int* __restrict__ out)
#if VELO_DEF_MATCH
{
    const MatchResJob& J = jobs[blockIdx.x];
    match_filter_job((int)blockIdx.x, J.n_query, J.n_train, J.q_out, keys, min_dist, match_thresh, total_q, out);
}
#else
;
#endif

}  // namespace velo
