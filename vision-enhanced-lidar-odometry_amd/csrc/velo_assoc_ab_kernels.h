// velo_assoc_ab_kernels.h -- the A/B kernels of the association family of velo_kernels.h (gfx950 / CDNA4 only): every launch of theirs is inside
// #ifdef VELO_DIAGNOSTICS, so velo_hip.hip and velo_unit_assoc.hip include this header in the diagnostics build only and the product
// library holds none of them.  They are the independent implementations the variant and parity tests compare the tube kernel against:
//   assoc_search_kernel                               VELO_ASSOC_VARIANT=0: one lane per query, the x-runs of its cell neighbourhood
//   assoc_search_v3_kernel                            the LDS-staged shrinking-radius box walk
//   assoc_lane_kernel / _batch_kernel                 VELO_ASSOC_LANE=1: one lane owns one query, for rounds that start from seeds
//   assoc_prepare_kernel + assoc_cluster_kernel       the pipelined form: one work item per cluster, persistent per-cluster search
#pragma once
#include "velo_kernels.h"

namespace velo {

// Reference association search (VELO_ASSOC_VARIANT=0, kept for A/B checks): one lane per query, each lane walks the
// x-runs of its own (2 reach + 1)^3 cell neighbourhood, reach = ceil(gate radius / cell).
__global__ void __launch_bounds__(kAssocThreads)
assoc_search_kernel(PoseScalars P, GridView G, const float4* __restrict__ src, const int* __restrict__ q_src, int q_begin, int q_end,
                    const float4* __restrict__ tgt, const int* __restrict__ tgt_off, const int* __restrict__ ring_of,
                    unsigned gate_bits, double norm_cond, int reach, AssocOut out, int want_aux)
#if VELO_DEF_ASSOC
{
    const int qi = q_begin + blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = qi < q_end;
    const unsigned long long key_inf = ((unsigned long long)gate_bits + 1ull) << 32;
    float4 psrc = make_float4(0.f, 0.f, 0.f, 0.f);
    float qx = 0.f, qy = 0.f, qz = 0.f;
    unsigned long long b1 = key_inf, b2 = key_inf;
    int b1ring = -1;
    if (active) {
        psrc = src[q_src[qi]];
        transform_query(P, psrc, &qx, &qy, &qz);
        const GridDesc& g = G.d;
        const int cx = cell_coord(qx, g.ox, g.inv_h, g.nx), cy = cell_coord(qy, g.oy, g.inv_h, g.ny), cz = cell_coord(qz, g.oz, g.inv_h, g.nz);
        const int x0 = max(cx - reach, 0), x1 = min(cx + reach, g.nx - 1);
        const int y0 = max(cy - reach, 0), y1 = min(cy + reach, g.ny - 1);
        const int z0 = max(cz - reach, 0), z1 = min(cz + reach, g.nz - 1);
        if (x0 <= x1) {
            for (int z = z0; z <= z1; z++) {
                for (int y = y0; y <= y1; y++) {
                    const int row = (z * g.ny + y);
                    const int j0 = grid_start(G, row, x0), j1 = grid_start(G, row, x1 + 1);
                    for (int j = j0; j < j1; j++) {
                        const float4 sp = G.sorted[j];
                        const float d2 = dist2_f(qx, qy, qz, sp.x, sp.y, sp.z);
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(sp.w);
                        if (key < b2) {                                  // implies d2 <= gate (keys start at key_inf)
                            const int ring = G.sring[j];
                            if (key < b1) {
                                if (ring != b1ring) b2 = b1;
                                b1 = key; b1ring = ring;
                            } else if (ring != b1ring) {
                                b2 = key;
                            }
                        }
                    }
                }
            }
        }
    }
    if (active) finish_correspondence(qi, psrc, qx, qy, qz, b1, b2, key_inf, tgt, tgt_off, ring_of, norm_cond, out, want_aux != 0);
}
#else
;
#endif

// ---- association search: LDS-staged shrinking-radius box walk (VELO_ASSOC_VARIANT=4; superseded by the tube kernel below, ----
// ---- kept for A/B and as the second independent implementation the parity tests compare against) ---------------------------
// A workgroup of NW waves owns 64 consecutive queries; lane i of EVERY wave holds query i (source scans are ring-ordered,
// so the 64 points are spatial neighbours).  The waves cluster the queries (cells within +-W of a seed lane's cell) and
// search ONE fine grid (cell ~ the smallest gate radius, shared by all outer iterations) in growing boxes around the
// cluster's cell bounding box: expansion e = 1, 2, 4, ... cells.  Per phase
//   1. one thread per grid row of the new shell reads the row's cell offsets (vector loads) -> list of candidate runs,
//      workgroup prefix sum of their lengths;
//   2. the runs are copied into an LDS tile by ALL threads with coalesced 16-byte loads (every thread finds its source
//      run by binary search in the LDS prefix array) -- hundreds of loads in flight instead of a dependent chain;
//   3. each wave sweeps a slice of the tile: the candidate is read from LDS with one broadcast ds_read_b128 and tested by
//      all 64 lanes (queries) at once;
//   4. the waves merge their per-lane (best1, best2) through LDS (top-2-distinct-rings is associative and idempotent).
// After a phase that covered expansion e every unvisited point is separated from every member query by >= e whole cells,
// so the walk stops once (e * cell)^2 > max over member lanes of b2d (second-best squared distance, or the gate when a
// lane has no second ring yet): no unvisited point can enter any lane's result.  In the dense part of a scan this ends
// after the first phase; the answer is still the exact exhaustive one.
// DBG = true compiles the diagnostic hooks selected at run time by `dbg` (bit 0/1/2: skip sweep / tiles / rows, 3: cycle stamps,
// 4: counters, 5: workgroup times, bits 8+: first expansion); the product instantiation has none of them -- they cost 56 spilled
// SGPRs and 9 spilled VGPRs when left in.
template <int NW, int MINW, bool DBG>
__global__ void __launch_bounds__(NW * 64, MINW)
assoc_search_v3_kernel(PoseScalars P, GridView G, const float4* __restrict__ src, const int* __restrict__ q_src, int q_begin, int q_end,
                       const float4* __restrict__ tgt, const int* __restrict__ tgt_off, const int* __restrict__ ring_of,
                       unsigned gate_bits, double norm_cond, int cluster_w, float h_safe, AssocOut out, int want_aux, int dbg, int xcd_map) {
    constexpr int NT = NW * 64;
    constexpr int NRUN = 2 * NT;                       // two run slots per row, NT rows per row chunk
    // tile: candidates stored as PAIRS -- {x0,x1,y0,y1} and {z0,z1,bits(g0),bits(g1)} -- so that the sweep handles two
    // candidates per packed-f32 instruction after two broadcast ds_read_b128
    __shared__ float4 s_xy[kTileCap / 2];
    __shared__ float4 s_zg[kTileCap / 2];
    __shared__ int s_ring[kTileCap];
    __shared__ int s_run_j0[NRUN];
    __shared__ int s_run_off[NRUN + 1];
    __shared__ int s_wave_tot[NW];
    __shared__ unsigned long long m1[NW][64], m2[NW][64];
    __shared__ int mr[NW][64];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    // diagnostic build only (DBG && (dbg & 8)): per-section cycle totals of wave 0, added to out.dbg[0..7]
    long long tacc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tlast = (DBG && (dbg & 8)) ? (long long)__builtin_readcyclecounter() : 0;
#define VELO_STAMP(k) do { if (DBG && (dbg & 8)) { const long long now__ = (long long)__builtin_readcyclecounter(); tacc[k] += now__ - tlast; tlast = now__; } } while (0)
    // XCD-aware group mapping: workgroups are dealt round-robin over the 8 XCDs, so blockIdx % 8 selects the XCD; give
    // each XCD one CONTIGUOUS eighth of the ring-ordered groups -- spatial neighbours then share that XCD's 4 MB L2
    // (cell table rows and candidate cells are re-read by adjacent groups).  Placement affects speed only.
    const int n_groups = (q_end - q_begin + 63) >> 6;
    const int per_xcd = (n_groups + 7) >> 3;
    const int group = xcd_map ? (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
    if (group >= n_groups || (xcd_map && (int)(blockIdx.x >> 3) >= per_xcd)) return;
    if ((DBG && (dbg & 32)) && threadIdx.x == 0) out.wg_times[2 * group] = __builtin_amdgcn_s_memrealtime();
    const int qi = q_begin + group * 64 + lane;
    const bool active = qi < q_end;
    const unsigned long long key_inf = ((unsigned long long)gate_bits + 1ull) << 32;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    Top2 t;
    t.b1 = key_inf; t.b2 = key_inf; t.b1ring = -1; t.b2ring = -1; t.b2d = __uint_as_float(gate_bits + 1u);
    const GridDesc g = G.d;
    int cx = 0, cy = 0, cz = 0;
    if (active) {
        const float4 psrc = src[q_src[qi]];                           // re-read at the end instead of living in 4 registers
        transform_query(P, psrc, &qx, &qy, &qz);
        cx = cell_coord(qx, g.ox, g.inv_h, g.nx); cy = cell_coord(qy, g.oy, g.inv_h, g.ny); cz = cell_coord(qz, g.oz, g.inv_h, g.nz);
    }
    VELO_STAMP(0);
    const f32x2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
    float* s_xy_f = reinterpret_cast<float*>(s_xy);
    float* s_zg_f = reinterpret_cast<float*>(s_zg);
    bool pending = active;
    for (;;) {                                                         // clusters (identical control flow in every wave)
        const unsigned long long pm = __ballot(pending);
        if (pm == 0ull) break;
        const int leader = (int)__ffsll((long long)pm) - 1;
        const int scx = __builtin_amdgcn_readlane(cx, leader), scy = __builtin_amdgcn_readlane(cy, leader), scz = __builtin_amdgcn_readlane(cz, leader);
        const bool member = pending && abs(cx - scx) <= cluster_w && abs(cy - scy) <= cluster_w && abs(cz - scz) <= cluster_w;
        const int big = 1 << 28;
        const int bx0 = __builtin_amdgcn_readfirstlane(wave_min_i(member ? cx : big)), bx1 = __builtin_amdgcn_readfirstlane(wave_max_i(member ? cx : -big));
        const int by0 = __builtin_amdgcn_readfirstlane(wave_min_i(member ? cy : big)), by1 = __builtin_amdgcn_readfirstlane(wave_max_i(member ? cy : -big));
        const int bz0 = __builtin_amdgcn_readfirstlane(wave_min_i(member ? cz : big)), bz1 = __builtin_amdgcn_readfirstlane(wave_max_i(member ? cz : -big));
        VELO_STAMP(1);
        if ((DBG && (dbg & 16)) && tid == 0) atomicAdd(&out.dbg[0], 1ull);
        int e_prev = -1;                                               // expansion already covered (-1: nothing yet)
        int e = DBG ? max(1, dbg >> 8) : 1;                                     // first expansion (tuning knob, default 1)
        for (;;) {                                                     // phases: e = 1, then (if needed) the reach the bounds demand
            // box of this phase (clipped) and of the previous one (unclipped; empty when e_prev < 0)
            const int X0 = max(bx0 - e, 0), X1 = min(bx1 + e, g.nx - 1);
            const int Y0 = max(by0 - e, 0), Y1 = min(by1 + e, g.ny - 1);
            const int Z0 = max(bz0 - e, 0), Z1 = min(bz1 + e, g.nz - 1);
            const int px0 = bx0 - e_prev, px1 = bx1 + e_prev, py0 = by0 - e_prev, py1 = by1 + e_prev, pz0 = bz0 - e_prev, pz1 = bz1 + e_prev;
            const int nyb = Y1 - Y0 + 1, nzb = Z1 - Z0 + 1;
            const int nrows = (X0 <= X1 && nyb > 0 && nzb > 0) ? nyb * nzb : 0;
            for (int rbase = 0; rbase < ((DBG && (dbg & 4)) ? 0 : nrows); rbase += NT) {          // row chunks (one row per thread)
                // ---- 1. run list ----
                int ja0 = 0, la = 0, jb0 = 0, lb = 0;
                const int r = rbase + tid;
                if (r < nrows) {
                    const int y = Y0 + r % nyb, z = Z0 + r / nyb;
                    const int row = (z * g.ny + y);
                    const bool fresh = e_prev < 0 || y < py0 || y > py1 || z < pz0 || z > pz1;
                    if (fresh) {
                        ja0 = grid_start(G, row, X0); la = grid_start(G, row, X1 + 1) - ja0;
                    } else {                                            // old row: only the cells left of px0 and right of px1 are new
                        const int a1 = min(px0 - 1, X1), b0 = max(px1 + 1, X0);
                        if (X0 <= a1) { ja0 = grid_start(G, row, X0); la = grid_start(G, row, a1 + 1) - ja0; }
                        if (b0 <= X1) { jb0 = grid_start(G, row, b0); lb = grid_start(G, row, X1 + 1) - jb0; }
                    }
                }
                // workgroup exclusive scan of (la + lb)
                const int mine = la + lb;
                int inc = mine;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(inc, off); if (lane >= off) inc += v; }
                if (lane == 63) s_wave_tot[wid] = inc;
                __syncthreads();
                int wbase = 0, total = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) { const int v = s_wave_tot[w]; if (w < wid) wbase += v; total += v; }
                const int ex = wbase + inc - mine;
                s_run_j0[2 * tid] = ja0; s_run_off[2 * tid] = ex;
                s_run_j0[2 * tid + 1] = jb0; s_run_off[2 * tid + 1] = ex + la;
                if (tid == 0) s_run_off[NRUN] = total;
                __syncthreads();
                VELO_STAMP(2);
                if ((DBG && (dbg & 16)) && tid == 0) { atomicAdd(&out.dbg[1], 1ull); atomicAdd(&out.dbg[2], (unsigned long long)total); if (e_prev >= 0) atomicAdd(&out.dbg[3], (unsigned long long)total); atomicAdd(&out.dbg[4], (unsigned long long)nrows); atomicAdd(&out.dbg[5], (unsigned long long)e); }
                if (DBG && (dbg & 2)) total = 0;
                // ---- 2./3. tiles ----
                for (int tbase = 0; tbase < total; tbase += kTileCap) {
                    const int tn = min(total - tbase, kTileCap);
                    const int tn2 = (tn + 1) & ~1;                     // the sweep consumes pairs
                    for (int i = tid; i < tn2; i += NT) {
                        float4 c = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), __int_as_float(0x7fffffff));
                        int cr = 0x7fffffff;
                        if (i < tn) {
                            const int slot = tbase + i;
                            int lo = 0;                                // largest k with s_run_off[k] <= slot (NRUN is a power of two)
#pragma unroll
                            for (int step = NRUN / 2; step > 0; step >>= 1) {
                                if (s_run_off[lo + step] <= slot) lo += step;
                            }
                            const int j = s_run_j0[lo] + (slot - s_run_off[lo]);
                            c = G.sorted[j];
                            cr = G.sring[j];
                        }
                        const int pr = i >> 1, hb = i & 1;
                        s_xy_f[4 * pr + hb] = c.x; s_xy_f[4 * pr + 2 + hb] = c.y;
                        s_zg_f[4 * pr + hb] = c.z; s_zg_f[4 * pr + 2 + hb] = c.w;
                        s_ring[i] = cr;
                    }
                    __syncthreads();
                    VELO_STAMP(3);
                    // each wave sweeps a contiguous slice of the tile's pairs for all 64 queries
                    const int npairs = tn2 >> 1;
                    const int per = (npairs + NW - 1) / NW;
                    const int p0 = wid * per, p1 = min(p0 + per, npairs);
                    if (member && !(DBG && (dbg & 1))) {
                        // 4 pairs (8 candidates) per trip: all LDS reads first, then the packed distance math, then the
                        // (rare) updates -- keeps 8 ds_read_b128 in flight instead of one dependent read per pair
                        int pi = p0;
                        for (; pi + 4 <= p1; pi += 4) {
                            float4 a[4], bq[4];
#pragma unroll
                            for (int u = 0; u < 4; u++) { a[u] = s_xy[pi + u]; bq[u] = s_zg[pi + u]; }
                            f32x2 d2[4];
#pragma unroll
                            for (int u = 0; u < 4; u++) {
                                const f32x2 cxp = {a[u].x, a[u].y}, cyp = {a[u].z, a[u].w}, czp = {bq[u].x, bq[u].y};
                                const f32x2 dx = qx2 - cxp, dy = qy2 - cyp, dz = qz2 - czp;
                                f32x2 d = dx * dx;                     // x -> y -> z accumulation, no FMA (-ffp-contract=off)
                                d = d + dy * dy;
                                d = d + dz * dz;
                                d2[u] = d;
                            }
                            float dmin = fminf(fminf(fminf(d2[0].x, d2[0].y), fminf(d2[1].x, d2[1].y)), fminf(fminf(d2[2].x, d2[2].y), fminf(d2[3].x, d2[3].y)));
                            if (dmin <= t.b2d) {                       // some candidate of the 8 may matter for this lane
#pragma unroll
                                for (int u = 0; u < 4; u++) {
                                    if (d2[u].x <= t.b2d) {
                                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2[u].x) << 32) | (unsigned)__float_as_int(bq[u].z);
                                        top2_update(t, key, s_ring[2 * (pi + u)]);
                                    }
                                    if (d2[u].y <= t.b2d) {
                                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2[u].y) << 32) | (unsigned)__float_as_int(bq[u].w);
                                        top2_update(t, key, s_ring[2 * (pi + u) + 1]);
                                    }
                                }
                            }
                        }
                        for (; pi < p1; pi++) {
                            const float4 a = s_xy[pi], bq = s_zg[pi];
                            const f32x2 cxp = {a.x, a.y}, cyp = {a.z, a.w}, czp = {bq.x, bq.y};
                            const f32x2 dx = qx2 - cxp, dy = qy2 - cyp, dz = qz2 - czp;
                            f32x2 d2 = dx * dx;
                            d2 = d2 + dy * dy;
                            d2 = d2 + dz * dz;
                            if (d2.x <= t.b2d) {
                                const unsigned long long key = ((unsigned long long)__float_as_uint(d2.x) << 32) | (unsigned)__float_as_int(bq.z);
                                top2_update(t, key, s_ring[2 * pi]);
                            }
                            if (d2.y <= t.b2d) {
                                const unsigned long long key = ((unsigned long long)__float_as_uint(d2.y) << 32) | (unsigned)__float_as_int(bq.w);
                                top2_update(t, key, s_ring[2 * pi + 1]);
                            }
                        }
                    }
                    VELO_STAMP(4);
                    __syncthreads();
                    VELO_STAMP(5);
                }
            }
            // ---- 4. merge across waves ----
            if (NW > 1) {
                m1[wid][lane] = t.b1; m2[wid][lane] = t.b2; mr[wid][lane] = t.b1ring;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    if (w == wid) continue;
                    const unsigned long long c1 = m1[w][lane], c2 = m2[w][lane];
                    if (c1 < t.b2) top2_update(t, c1, mr[w][lane]);
                    if (c2 < t.b2) top2_update(t, c2, ring_of[(int)(unsigned)(c2 & 0xffffffffull) - out.first_point]);
                }
                __syncthreads();
            }
            // ---- stop test (identical in every wave: all hold the same merged state) ----
            // Every unvisited point is separated from every member query by >= e whole cells.  b2d only shrinks, so the
            // radius the CURRENT bounds allow is enough for one more phase to finish the cluster.
            const float rw = __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane(wave_max_i(member ? (int)__float_as_uint(t.b2d) : 0)));
            const float reach = (float)e * h_safe;
            VELO_STAMP(6);
            if (reach * reach > rw) break;
            e_prev = e;
            e = max(e + 1, (int)ceilf(sqrtf(rw) / h_safe));
            if ((float)e * h_safe * ((float)e * h_safe) <= rw) e++;     // rounding guard: the next test must pass
        }
        pending = pending && !member;
    }
    if (NW > 1 && wid != 0) return;
    if (active) finish_correspondence(qi, src[q_src[qi]], qx, qy, qz, t.b1, t.b2, key_inf, tgt, tgt_off, ring_of, norm_cond, out, want_aux != 0);
    VELO_STAMP(7);
    if ((DBG && (dbg & 32)) && tid == 0) out.wg_times[2 * group + 1] = __builtin_amdgcn_s_memrealtime();
    if ((DBG && (dbg & 8)) && tid == 0) { for (int k = 0; k < 8; k++) atomicAdd((unsigned long long*)&out.dbg[k], (unsigned long long)tacc[k]); }
#undef VELO_STAMP
}

// ---- association search, lane variant: the rounds that start from seeds ------------------------------------------------------
// The tube kernel shares every staged candidate among the 64 queries of a group: 350 candidates x 64 lanes per warm round, of
// which a query needs the ~15 of its own bound sphere -- 9,400 lane-instructions per query.  A round that starts from the
// previous round's winners knows a tight bound for (nearly) every query BEFORE it looks at a single cell, so sharing buys
// nothing: here ONE LANE OWNS ONE QUERY and walks the cells of its own bound sphere straight from the cell-sorted copy in L2
// (neighbouring lanes walk neighbouring cells, so the gathers share lines).  No tile, no run list of the group, no workgroup
// barrier -- a workgroup is four independent waves.
//   * easy query (bound box <= 3 x 3 rows, the rule whenever the bound is below one cell): the lane fetches the (start, end)
//     of its <= 9 row runs at once, keeps the non-empty ones in its LDS column and then consumes them four candidates per trip
//     (all four loads in flight together; entries behind the end of a run are real points of the next cells or the +inf
//     sentinels behind the last point -- harmless extra candidates);
//   * hard query (a query whose second ring is farther than a cell: no second seed, first iteration's gate = 4 cells): the
//     wave turns all 64 lanes on that one query, as the tube kernel's asker phase does (rows over lanes -> wave prefix sum ->
//     candidates over lanes -> xor-shuffle merge).
// Candidate set = every point of every cell the bound sphere touches, keys and tie rules as everywhere else: the tables equal the
// tube kernel's bit for bit (tests: warm rounds against cold rounds, against the oracle, lane against tube).
// MEASURED (C2, one pair in flight): 88-90 us per second-iteration round against the tube kernel's 46-50, 440 us per seeded
// first-iteration round (10-25 % hard queries, each a 9 x 9-row box) against 80.  The instruction count is what was hoped for, but
// every lane-private 16-byte gather pulls a 128-byte line from L2 into a 16 KB L1 that 64 lanes x 8 gathers per trip thrash: the
// kernel waits on L2->L1 line traffic (~0.8 MB per wave) that the tube kernel's coalesced staging never creates.  Kept as an
// independent second implementation for the parity tests and as an A/B (VELO_ASSOC_LANE=1), NOT the default.
template <bool DBG>
__device__ __forceinline__ void
assoc_lane_body(const PoseScalars& P_in, const PoseRecord* __restrict__ P_dev, int* __restrict__ chain_fail, const GridView& G, const float4* __restrict__ qpts, int q_begin, int q_end,
                const float4* __restrict__ tgt_pad, const int* __restrict__ tgt_off, unsigned gate_bits, double norm_cond, const AssocOut& out, int want_aux, const int block_x) {
    constexpr int kRows = 9;
    __shared__ int s_j0[4][kRows][64];
    __shared__ int s_j1[4][kRows][64];
    __shared__ int s_cj0[4][66];
    __shared__ int s_coff[4][66];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (chain_fail && *chain_fail) return;
    if (P_dev && !P_dev->ready) { if (block_x == 0 && tid == 0) *chain_fail = 1; return; }
    const PoseScalars& P = P_dev ? P_dev->P : P_in;
    if (out.n_valid_next && block_x == 0 && tid == 0) *out.n_valid_next = 0;
    const int group = block_x * 4 + wid;
    if (group * 64 >= q_end - q_begin) return;                         // wave-uniform
    const int qi = q_begin + group * 64 + lane;
    const bool active = qi < q_end;
    const unsigned long long key_inf = ((unsigned long long)gate_bits + 1ull) << 32;
    Top2 t;
    t.b1 = key_inf; t.b2 = key_inf; t.b1ring = -1; t.b2ring = -1; t.b2d = __uint_as_float(gate_bits + 1u);
    const GridDesc g = G.d;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    if (active) {
        const float4 psrc = qpts[qi];
        const float4 sa = out.prev_a[qi], sb = out.prev_b[qi];
        const int2 sr = out.prev_r[qi];
        transform_query(P, psrc, &qx, &qy, &qz);
        if (__float_as_int(sa.w) >= 0) {
            const float d = dist2_f(sa.x, sa.y, sa.z, qx, qy, qz);
            if (__float_as_uint(d) <= gate_bits) top2_update(t, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(__float_as_int(sa.w) + out.first_point), sr.x);
        }
        if (__float_as_int(sb.w) >= 0) {
            const float d = dist2_f(sb.x, sb.y, sb.z, qx, qy, qz);
            if (__float_as_uint(d) <= gate_bits) top2_update(t, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(__float_as_int(sb.w) + out.first_point), sr.y);
        }
    }
    // the cell box of the bound sphere (padded against rounding, like the tube kernel's)
    const float r0 = sqrtf(t.b2d) * 1.0001f + 1e-6f;
    int x0, x1, y0, y1, z0, z1;
    {
        const CellBox bb = query_box(g, qx, qy, qz, 0, 0, 0, r0, false);
        x0 = max(bb.x0, 0); x1 = min(bb.x1, g.nx - 1); y0 = max(bb.y0, 0); y1 = min(bb.y1, g.ny - 1); z0 = max(bb.z0, 0); z1 = min(bb.z1, g.nz - 1);
    }
    const int nyb = y1 - y0 + 1, nzb = z1 - z0 + 1;
    const bool some = active && x0 <= x1 && nyb > 0 && nzb > 0;        // else: the sphere lies outside the grid, nothing to look at
    const bool easy = some && nyb <= 3 && nzb <= 3;
    const bool hard = some && !easy;
    // ---- easy lanes: own row runs -> LDS column -> four candidates per trip ----
    int nrun = 0;
    if (easy) {
        int a[kRows], b[kRows];
#pragma unroll
        for (int zz = 0; zz < 3; zz++) {
#pragma unroll
            for (int yy = 0; yy < 3; yy++) {
                const bool on = zz < nzb && yy < nyb;
                const int row = on ? ((z0 + zz) * g.ny + (y0 + yy)) : 0;
                a[zz * 3 + yy] = on ? grid_start(G, row, x0) : 0;
                b[zz * 3 + yy] = on ? grid_start(G, row, x1 + 1) : 0;
            }
        }
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            if (b[k] > a[k]) { s_j0[wid][nrun][lane] = a[k]; s_j1[wid][nrun][lane] = b[k]; nrun++; }
        }
    }
    {
        int k = 0, j = 0, jend = 0;
        for (;;) {
            if (j >= jend && k < nrun) { j = s_j0[wid][k][lane]; jend = s_j1[wid][k][lane]; k++; }
            const bool have = j < jend;
            if (__ballot(have) == 0ull) break;
            const int jj = have ? j : 0;
            const float4 c0 = G.sorted[jj], c1 = G.sorted[jj + 1], c2 = G.sorted[jj + 2], c3 = G.sorted[jj + 3];
            const int g0 = G.sring[jj], g1 = G.sring[jj + 1], g2 = G.sring[jj + 2], g3 = G.sring[jj + 3];
            const float d0 = dist2_f(qx, qy, qz, c0.x, c0.y, c0.z), d1 = dist2_f(qx, qy, qz, c1.x, c1.y, c1.z);
            const float d2 = dist2_f(qx, qy, qz, c2.x, c2.y, c2.z), d3 = dist2_f(qx, qy, qz, c3.x, c3.y, c3.z);
            if (have && fminf(fminf(d0, d1), fminf(d2, d3)) <= t.b2d) {
                if (d0 <= t.b2d) top2_update(t, ((unsigned long long)__float_as_uint(d0) << 32) | (unsigned)__float_as_int(c0.w), g0);
                if (d1 <= t.b2d) top2_update(t, ((unsigned long long)__float_as_uint(d1) << 32) | (unsigned)__float_as_int(c1.w), g1);
                if (d2 <= t.b2d) top2_update(t, ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(c2.w), g2);
                if (d3 <= t.b2d) top2_update(t, ((unsigned long long)__float_as_uint(d3) << 32) | (unsigned)__float_as_int(c3.w), g3);
            }
            j += 4;
        }
    }
    // ---- hard lanes: the whole wave on one query at a time ----
    unsigned long long hm = __ballot(hard);
    while (hm != 0ull) {
        const int la = (int)__ffsll((long long)hm) - 1;
        hm &= hm - 1ull;
        const float ax = __shfl(qx, la), ay = __shfl(qy, la), az = __shfl(qz, la);
        Top2 tl;
        tl.b1 = __shfl(t.b1, la); tl.b2 = __shfl(t.b2, la); tl.b1ring = __shfl(t.b1ring, la); tl.b2ring = __shfl(t.b2ring, la);
        tl.b2d = __uint_as_float((unsigned)(tl.b2 >> 32));
        const int bx0 = __shfl(x0, la), bx1 = __shfl(x1, la), by0 = __shfl(y0, la), bz0 = __shfl(z0, la);
        const int ny = __shfl(nyb, la), nz = __shfl(nzb, la);
        const int nrows_a = ny * nz;
        const float rcp_ny = 1.0f / (float)ny;
        for (int rb = 0; rb < nrows_a; rb += 64) {
            const int r = rb + lane;
            int j0 = 0, len = 0;
            if (r < nrows_a) {
                int zq = (int)((float)r * rcp_ny), yr = r - zq * ny;
                if (yr < 0) { zq--; yr += ny; } else if (yr >= ny) { zq++; yr -= ny; }
                const int row = ((bz0 + zq) * g.ny + (by0 + yr));
                j0 = grid_start(G, row, bx0); len = grid_start(G, row, bx1 + 1) - j0;
            }
            int inc = len;
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(inc, off); if (lane >= off) inc += v; }
            const int total = __shfl(inc, 63);
            s_cj0[wid][lane] = j0; s_coff[wid][lane] = inc - len;
            if (lane == 0) s_coff[wid][64] = total;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (int slot = lane; slot < total; slot += 64) {
                int lo = 0;                                            // largest i with s_coff[i] <= slot
#pragma unroll
                for (int step = 32; step > 0; step >>= 1) { if (s_coff[wid][lo + step] <= slot) lo += step; }
                const int j = s_cj0[wid][lo] + (slot - s_coff[wid][lo]);
                const float4 c = G.sorted[j];
                const float d = dist2_f(ax, ay, az, c.x, c.y, c.z);
                if (d <= tl.b2d) top2_update(tl, ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(c.w), G.sring[j]);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();                           // the run list is rewritten by the next rows
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) top2_merge_xor(tl, m);
        if (lane == la) { t.b1 = tl.b1; t.b2 = tl.b2; t.b1ring = tl.b1ring; t.b2ring = tl.b2ring; t.b2d = tl.b2d; }
    }
    if (active) finish_correspondence_pad(qi, qpts, qx, qy, qz, t.b1, t.b2, t.b1ring, t.b2ring, key_inf, tgt_pad, tgt_off, norm_cond, out, want_aux != 0);
}

__global__ void __launch_bounds__(256)
assoc_lane_kernel(PoseScalars P, const PoseRecord* __restrict__ P_dev, int* __restrict__ chain_fail, GridView G, const float4* __restrict__ qpts, int q_begin, int q_end,
                  const float4* __restrict__ tgt_pad, const int* __restrict__ tgt_off, unsigned gate_bits, double norm_cond, AssocOut out, int want_aux)
#if VELO_DEF_ASSOC
{
    assoc_lane_body<false>(P, P_dev, chain_fail, G, qpts, q_begin, q_end, tgt_pad, tgt_off, gate_bits, norm_cond, out, want_aux, (int)blockIdx.x);
}
#else
;
#endif
// the same round of several contexts in one launch (blockIdx.y = context)
__global__ void __launch_bounds__(256)
assoc_lane_batch_kernel(AssocBatch B)
#if VELO_DEF_ASSOC
{
    const AssocArgs& a = B.item[blockIdx.y];
    if ((int)blockIdx.x * 256 >= a.q_end - a.q_begin) return;
    assoc_lane_body<false>(a.P, a.P_dev, a.chain_fail, a.G, a.qpts, a.q_begin, a.q_end, a.tgt_pad, a.tgt_off, a.gate_bits, a.norm_cond, a.out, a.want_aux, (int)blockIdx.x);
}
#else
;
#endif

// ---- association as a balanced pipeline: prepare (clusters -> work items) + persistent per-cluster search -----------------
// The monolithic kernel above walks a group's clusters one after the other, so a 64-query group with several clusters and
// two phases each is a long latency chain while most workgroups have already left.  Here a cheap prepare kernel (one
// wave per group) transforms the queries, forms the clusters and appends ONE WORK ITEM PER CLUSTER; a persistent kernel
// then keeps every workgroup slot busy: workgroups pull items from a global queue, run that cluster's phases (same LDS
// staged box walk) and finish the correspondences of the cluster's member lanes.
// The queue is split into kQShards sub-queues (one returning atomic on ONE word tops out near 90 per microsecond on
// this chip): group g appends to shard g % kQShards with a single reservation, a workgroup pulls from shard
// blockIdx % kQShards first and steals from the others when its own runs dry.  Counters sit on separate 128-byte lines.
constexpr int kQShards = 8;
constexpr int kQStride = 32;         // ints between counters
struct AssocQueue {
    AssocItem* __restrict__ items;   // kQShards regions of shard_cap items
    int shard_cap;
    int* __restrict__ counters;      // [s * kQStride] = items in shard s, [(kQShards + s) * kQStride] = dequeue head of shard s
    float4* __restrict__ qpos;       // transformed query coordinates (float, as the reference rounds them) per query
};

__global__ void __launch_bounds__(64)
assoc_prepare_kernel(PoseScalars P, GridDesc g, const float4* __restrict__ src, const int* __restrict__ q_src, int q_begin, int q_end,
                     int cluster_w, AssocQueue Q)
#if VELO_DEF_ASSOC
{
    const int lane = threadIdx.x;
    const int group = blockIdx.x;
    const int qi = q_begin + group * 64 + lane;
    const bool active = qi < q_end;
    float qx = 0.f, qy = 0.f, qz = 0.f;
    int cx = 0, cy = 0, cz = 0;
    if (active) {
        const float4 psrc = src[q_src[qi]];
        transform_query(P, psrc, &qx, &qy, &qz);
        cx = cell_coord(qx, g.ox, g.inv_h, g.nx); cy = cell_coord(qy, g.oy, g.inv_h, g.ny); cz = cell_coord(qz, g.oz, g.inv_h, g.nz);
        Q.qpos[qi] = make_float4(qx, qy, qz, 0.f);
    }
    // pass 1: count this group's clusters; one reservation per group in its shard
    int n_clusters = 0;
    {
        bool pending = active;
        for (;;) {
            const unsigned long long pm = __ballot(pending);
            if (pm == 0ull) break;
            const int leader = (int)__ffsll((long long)pm) - 1;
            const int scx = __builtin_amdgcn_readlane(cx, leader), scy = __builtin_amdgcn_readlane(cy, leader), scz = __builtin_amdgcn_readlane(cz, leader);
            const bool member = pending && abs(cx - scx) <= cluster_w && abs(cy - scy) <= cluster_w && abs(cz - scz) <= cluster_w;
            n_clusters++;
            pending = pending && !member;
        }
    }
    const int shard = group % kQShards;
    int base = 0;
    if (lane == 0 && n_clusters > 0) base = atomicAdd(&Q.counters[shard * kQStride], n_clusters);
    base = __builtin_amdgcn_readfirstlane(base);
    // pass 2: write the items
    bool pending = active;
    int k = 0;
    for (;;) {
        const unsigned long long pm = __ballot(pending);
        if (pm == 0ull) break;
        const int leader = (int)__ffsll((long long)pm) - 1;
        const int scx = __builtin_amdgcn_readlane(cx, leader), scy = __builtin_amdgcn_readlane(cy, leader), scz = __builtin_amdgcn_readlane(cz, leader);
        const bool member = pending && abs(cx - scx) <= cluster_w && abs(cy - scy) <= cluster_w && abs(cz - scz) <= cluster_w;
        const unsigned long long mm = __ballot(member);
        const int big = 1 << 28;
        const int bx0 = wave_min_i(member ? cx : big), bx1 = wave_max_i(member ? cx : -big);
        const int by0 = wave_min_i(member ? cy : big), by1 = wave_max_i(member ? cy : -big);
        const int bz0 = wave_min_i(member ? cz : big), bz1 = wave_max_i(member ? cz : -big);
        if (lane == 0) {
            AssocItem it;
            it.group = group; it.mask_lo = (unsigned)(mm & 0xffffffffull); it.mask_hi = (unsigned)(mm >> 32);
            // cell coordinates live in [-2, n+1] with n <= 8192: bias by 2 and pack two 16-bit fields
            it.bx = (bx0 + 2) | ((bx1 + 2) << 16); it.by = (by0 + 2) | ((by1 + 2) << 16); it.bz = (bz0 + 2) | ((bz1 + 2) << 16);
            it.pad0 = 0; it.pad1 = 0;
            Q.items[(size_t)shard * Q.shard_cap + base + k] = it;
        }
        k++;
        pending = pending && !member;
    }
}
#else
;
#endif

template <int NW, int MINW>
__global__ void __launch_bounds__(NW * 64, MINW)
assoc_cluster_kernel(GridView G, AssocQueue Q, const float4* __restrict__ src, const int* __restrict__ q_src, int q_begin, int q_end,
                     const float4* __restrict__ tgt, const int* __restrict__ tgt_off, const int* __restrict__ ring_of,
                     unsigned gate_bits, double norm_cond, float h_safe, AssocOut out, int want_aux) {
    constexpr int NT = NW * 64;
    constexpr int NRUN = 2 * NT;
    __shared__ float4 s_xy[kTileCap / 2];
    __shared__ float4 s_zg[kTileCap / 2];
    __shared__ int s_ring[kTileCap];
    __shared__ int s_run_j0[NRUN];
    __shared__ int s_run_off[NRUN + 1];
    __shared__ int s_wave_tot[NW];
    __shared__ unsigned long long m1[NW][64], m2[NW][64];
    __shared__ int mr[NW][64];
    __shared__ int s_item;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long key_inf = ((unsigned long long)gate_bits + 1ull) << 32;
    const GridDesc g = G.d;
    float* s_xy_f = reinterpret_cast<float*>(s_xy);
    float* s_zg_f = reinterpret_cast<float*>(s_zg);
    int shard = blockIdx.x % kQShards, tries = 0;

    for (;;) {                                                         // persistent: pull the next cluster
        if (tid == 0) {
            int got = -1;
            while (tries < kQShards) {
                const int n = Q.counters[shard * kQStride];
                int* head = &Q.counters[(kQShards + shard) * kQStride];
                // plain peek first: an exhausted shard costs no atomic
                if (__hip_atomic_load(head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < n) {
                    const int h = atomicAdd(head, 1);
                    if (h < n) { got = shard * Q.shard_cap + h; break; }
                }
                shard = (shard + 1) % kQShards; tries++;
            }
            s_item = got;
        }
        __syncthreads();
        const int item = s_item;
        __syncthreads();
        if (item < 0) break;
        const AssocItem it = Q.items[item];
        const unsigned long long mm = ((unsigned long long)it.mask_hi << 32) | it.mask_lo;
        const bool member = (mm >> lane) & 1ull;
        const int qi = q_begin + it.group * 64 + lane;
        const int bx0 = (it.bx & 0xffff) - 2, bx1 = (it.bx >> 16) - 2;
        const int by0 = (it.by & 0xffff) - 2, by1 = (it.by >> 16) - 2;
        const int bz0 = (it.bz & 0xffff) - 2, bz1 = (it.bz >> 16) - 2;
        float qx = 0.f, qy = 0.f, qz = 0.f;
        if (member) { const float4 qp = Q.qpos[qi]; qx = qp.x; qy = qp.y; qz = qp.z; }
        const f32x2 qx2 = {qx, qx}, qy2 = {qy, qy}, qz2 = {qz, qz};
        Top2 t;
        t.b1 = key_inf; t.b2 = key_inf; t.b1ring = -1; t.b2ring = -1; t.b2d = __uint_as_float(gate_bits + 1u);
        int e_prev = -1, e = 1;
        for (;;) {                                                     // phases (see assoc_search_v3_kernel)
            const int X0 = max(bx0 - e, 0), X1 = min(bx1 + e, g.nx - 1);
            const int Y0 = max(by0 - e, 0), Y1 = min(by1 + e, g.ny - 1);
            const int Z0 = max(bz0 - e, 0), Z1 = min(bz1 + e, g.nz - 1);
            const int px0 = bx0 - e_prev, px1 = bx1 + e_prev, py0 = by0 - e_prev, py1 = by1 + e_prev, pz0 = bz0 - e_prev, pz1 = bz1 + e_prev;
            const int nyb = Y1 - Y0 + 1, nzb = Z1 - Z0 + 1;
            const int nrows = (X0 <= X1 && nyb > 0 && nzb > 0) ? nyb * nzb : 0;
            const float inv_nyb = 1.0f / (float)max(nyb, 1);
            for (int rbase = 0; rbase < nrows; rbase += NT) {
                int ja0 = 0, la = 0, jb0 = 0, lb = 0;
                const int r = rbase + tid;
                if (r < nrows) {
                    int zq = (int)(((float)r + 0.5f) * inv_nyb);      // r / nyb for small non-negative ints, fixed up below
                    zq = (zq * nyb > r) ? zq - 1 : ((zq + 1) * nyb <= r ? zq + 1 : zq);
                    const int y = Y0 + (r - zq * nyb), z = Z0 + zq;
                    const int row = (z * g.ny + y);
                    const bool fresh = e_prev < 0 || y < py0 || y > py1 || z < pz0 || z > pz1;
                    if (fresh) {
                        ja0 = grid_start(G, row, X0); la = grid_start(G, row, X1 + 1) - ja0;
                    } else {
                        const int a1 = min(px0 - 1, X1), b0 = max(px1 + 1, X0);
                        if (X0 <= a1) { ja0 = grid_start(G, row, X0); la = grid_start(G, row, a1 + 1) - ja0; }
                        if (b0 <= X1) { jb0 = grid_start(G, row, b0); lb = grid_start(G, row, X1 + 1) - jb0; }
                    }
                }
                const int mine = la + lb;
                int inc = mine;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(inc, off); if (lane >= off) inc += v; }
                if (lane == 63) s_wave_tot[wid] = inc;
                __syncthreads();
                int wbase = 0, total = 0;
#pragma unroll
                for (int w = 0; w < NW; w++) { const int v = s_wave_tot[w]; if (w < wid) wbase += v; total += v; }
                const int ex = wbase + inc - mine;
                s_run_j0[2 * tid] = ja0; s_run_off[2 * tid] = ex;
                s_run_j0[2 * tid + 1] = jb0; s_run_off[2 * tid + 1] = ex + la;
                if (tid == 0) s_run_off[NRUN] = total;
                __syncthreads();
                for (int tbase = 0; tbase < total; tbase += kTileCap) {
                    const int tn = min(total - tbase, kTileCap);
                    const int tn8 = (tn + 7) & ~7;                     // the sweep consumes 4 pairs per trip
                    for (int i = tid; i < tn8; i += NT) {
                        float4 c = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), __int_as_float(0x7fffffff));
                        int cr = 0x7fffffff;
                        if (i < tn) {
                            const int slot = tbase + i;
                            int lo = 0;
#pragma unroll
                            for (int step = NRUN / 2; step > 0; step >>= 1) {
                                if (s_run_off[lo + step] <= slot) lo += step;
                            }
                            const int j = s_run_j0[lo] + (slot - s_run_off[lo]);
                            c = G.sorted[j];
                            cr = G.sring[j];
                        }
                        const int pr = i >> 1, hb = i & 1;
                        s_xy_f[4 * pr + hb] = c.x; s_xy_f[4 * pr + 2 + hb] = c.y;
                        s_zg_f[4 * pr + hb] = c.z; s_zg_f[4 * pr + 2 + hb] = c.w;
                        s_ring[i] = cr;
                    }
                    __syncthreads();
                    const int nquads = tn8 >> 3;                       // groups of 4 pairs
                    const int per = (nquads + NW - 1) / NW;
                    const int g0 = wid * per, g1 = min(g0 + per, nquads);
                    if (member) {
                        for (int gq = g0; gq < g1; gq++) {
                            const int pi = gq * 4;
                            float4 a[4], bq[4];
#pragma unroll
                            for (int u = 0; u < 4; u++) { a[u] = s_xy[pi + u]; bq[u] = s_zg[pi + u]; }
                            f32x2 d2[4];
#pragma unroll
                            for (int u = 0; u < 4; u++) {
                                const f32x2 cxp = {a[u].x, a[u].y}, cyp = {a[u].z, a[u].w}, czp = {bq[u].x, bq[u].y};
                                const f32x2 dx = qx2 - cxp, dy = qy2 - cyp, dz = qz2 - czp;
                                f32x2 d = dx * dx;                     // x -> y -> z accumulation, no FMA (-ffp-contract=off)
                                d = d + dy * dy;
                                d = d + dz * dz;
                                d2[u] = d;
                            }
                            const float dmin = fminf(fminf(fminf(d2[0].x, d2[0].y), fminf(d2[1].x, d2[1].y)), fminf(fminf(d2[2].x, d2[2].y), fminf(d2[3].x, d2[3].y)));
                            if (dmin <= t.b2d) {
#pragma unroll
                                for (int u = 0; u < 4; u++) {
                                    if (d2[u].x <= t.b2d) {
                                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2[u].x) << 32) | (unsigned)__float_as_int(bq[u].z);
                                        top2_update(t, key, s_ring[2 * (pi + u)]);
                                    }
                                    if (d2[u].y <= t.b2d) {
                                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2[u].y) << 32) | (unsigned)__float_as_int(bq[u].w);
                                        top2_update(t, key, s_ring[2 * (pi + u) + 1]);
                                    }
                                }
                            }
                        }
                    }
                    __syncthreads();
                }
            }
            if (NW > 1) {
                m1[wid][lane] = t.b1; m2[wid][lane] = t.b2; mr[wid][lane] = t.b1ring;
                __syncthreads();
#pragma unroll
                for (int w = 0; w < NW; w++) {
                    if (w == wid) continue;
                    const unsigned long long c1 = m1[w][lane], c2 = m2[w][lane];
                    if (c1 < t.b2) top2_update(t, c1, mr[w][lane]);
                    if (c2 < t.b2) top2_update(t, c2, ring_of[(int)(unsigned)(c2 & 0xffffffffull) - out.first_point]);
                }
                __syncthreads();
            }
            const float rw = __uint_as_float((unsigned)__builtin_amdgcn_readfirstlane(wave_max_i(member ? (int)__float_as_uint(t.b2d) : 0)));
            const float reach = (float)e * h_safe;
            if (reach * reach > rw) break;
            e_prev = e;
            e = max(e + 1, (int)ceilf(sqrtf(rw) / h_safe));
            if ((float)e * h_safe * ((float)e * h_safe) <= rw) e++;
        }
        // rows A3-A6 for the member lanes of this cluster (wave 0 holds the merged state like every other wave)
        if (wid == 0 && member && qi < q_end) {
            const float4 psrc = src[q_src[qi]];
            finish_correspondence(qi, psrc, qx, qy, qz, t.b1, t.b2, key_inf, tgt, tgt_off, ring_of, norm_cond, out, want_aux != 0);
        }
    }
}

// ---- template kernels: instantiated by the unit that owns the family, `extern template` for everybody else --------------------------------
#define VELO_V3_ARGS (PoseScalars, GridView, const float4*, const int*, int, int, const float4*, const int*, const int*, unsigned, double, int, float, AssocOut, int, int, int)
#define VELO_CLUSTER_ARGS (GridView, AssocQueue, const float4*, const int*, int, int, const float4*, const int*, const int*, unsigned, double, float, AssocOut, int)
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<1, 1, false> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<1, 1, true> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<2, 1, false> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<2, 1, true> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<4, 5, false> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<4, 5, true> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<4, 6, false> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<4, 6, true> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<4, 7, false> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<4, 7, true> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<4, 8, false> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<4, 8, true> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<8, 8, false> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_search_v3_kernel<8, 8, true> VELO_V3_ARGS;
VELO_INST_ASSOC __global__ void assoc_cluster_kernel<2, 1> VELO_CLUSTER_ARGS;
VELO_INST_ASSOC __global__ void assoc_cluster_kernel<4, 6> VELO_CLUSTER_ARGS;
VELO_INST_ASSOC __global__ void assoc_cluster_kernel<8, 6> VELO_CLUSTER_ARGS;
#undef VELO_V3_ARGS
#undef VELO_CLUSTER_ARGS

}  // namespace velo
