// velo_host_types.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  Error state, device buffers, the search index, TargetData and velo_ctx: what one context holds.
namespace {

thread_local std::string g_err;
std::string g_err_shared;   // last error of any thread (read by velo_last_error when the caller's own is empty)
std::mutex g_err_mutex;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    { std::lock_guard<std::mutex> lk(g_err_mutex); g_err_shared = buf; }
    return code;
}

#ifdef VELO_DIAGNOSTICS
// dev aid (VELO_API_TRACE=<us>, diagnostics build): every runtime call that keeps its caller longer than that is reported with its text --
// how the copies that block for milliseconds were found.  Synchronisations are expected to wait and are not reported.
static const double g_api_trace_us = getenv("VELO_API_TRACE") ? atof(getenv("VELO_API_TRACE")) : 0.0;
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        const auto t__ = g_api_trace_us > 0.0 ? std::chrono::steady_clock::now() : std::chrono::steady_clock::time_point(); \
        hipError_t e__ = (expr);                                                                        \
        if (g_api_trace_us > 0.0) {                                                                     \
            const double us__ = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t__).count(); \
            if (us__ > g_api_trace_us && !strstr(#expr, "Synchronize")) fprintf(stderr, "[velo api] %.0f us in %s (line %d)\n", us__, #expr, __LINE__); \
        }                                                                                               \
        if (e__ != hipSuccess) return fail(VELO_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)
#else
#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) return fail(VELO_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)
#endif
#define NCCL_TRY(expr)                                                                                  \
    do {                                                                                                \
        ncclResult_t r__ = (expr);                                                                      \
        if (r__ != ncclSuccess) return fail(VELO_ERR_COMM, "%s failed: %s (%s:%d)", #expr, ncclGetErrorString(r__), __FILE__, __LINE__); \
    } while (0)
#define VELO_TRY(expr)           \
    do {                         \
        int s__ = (expr);        \
        if (s__ != VELO_OK) return s__; \
    } while (0)

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { release(); }             // every buffer a context owns goes with it: velo_destroy is `delete c` and lists none of them
    int reserve(size_t n) {
        if (n <= cap) return VELO_OK;
        const size_t cap_before = cap; (void)cap_before;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        size_t want = n + n / 8 + 64;
#ifdef VELO_DIAGNOSTICS
        // A/B (VELO_ALLOC_2MB=1): buffers of 256 KB and more padded to whole 2 MB -- does the page-table fragment size matter to the gathers?
        static const bool pad2m = getenv("VELO_ALLOC_2MB") && atoi(getenv("VELO_ALLOC_2MB")) != 0;
        if (pad2m && want * sizeof(T) >= (256u << 10)) want = ((want * sizeof(T) + (2u << 20) - 1) / (2u << 20)) * (2u << 20) / sizeof(T);
#endif
#ifdef VELO_DIAGNOSTICS
        static const bool alloc_trace = getenv("VELO_ALLOC_TRACE") != nullptr;   // dev aid: a (re)allocation synchronises the device -- which buffers still grow in a warm loop?
        if (alloc_trace) fprintf(stderr, "[velo alloc] device buffer of %zu-byte elements: %zu -> %zu elements\n", sizeof(T), cap_before, want);
#endif
        hipError_t e = hipMalloc((void**)&p, want * sizeof(T));
        if (e != hipSuccess) return fail(VELO_ERR_HIP, "hipMalloc(%zu bytes) failed: %s", want * sizeof(T), hipGetErrorString(e));
        cap = want;
        return VELO_OK;
    }
    // for buffers whose size moves from frame to frame (the index table follows the scan's bounding box): when it has to grow, grow by `extra`
    // elements more -- a reallocation synchronises the device, and the queues stall for 6-7 ms one step later (measured: tools/step_times.py)
    int reserve_roomy(size_t n, size_t extra) { return n <= cap ? VELO_OK : reserve(n + extra); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// page-locked host memory, owned like a device buffer: staging of uploads and landing of read-backs.  Sized in bytes; a buffer that
// grows is freed first (its contents are not kept), and the owner sees to it that no copy is in flight when it asks for more.
template <typename T = unsigned char>
struct PinBuf {
    T* p = nullptr;
    size_t cap = 0;                      // bytes
    PinBuf() = default;
    PinBuf(const PinBuf&) = delete;
    PinBuf& operator=(const PinBuf&) = delete;
    PinBuf(PinBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinBuf& operator=(PinBuf&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~PinBuf() { release(); }
    int reserve(size_t bytes) {
        if (bytes <= cap) return VELO_OK;
        const size_t want = bytes + bytes / 4 + 4096;
#ifdef VELO_DIAGNOSTICS
        static const bool alloc_trace = getenv("VELO_ALLOC_TRACE") != nullptr;   // dev aid, as in DevBuf::reserve: which pinned buffers still grow in a warm loop?
        if (alloc_trace) fprintf(stderr, "[velo alloc] pinned buffer: %zu -> %zu bytes\n", cap, want);
#endif
        release();
        HIP_TRY(hipHostMalloc((void**)&p, want, hipHostMallocDefault));
        cap = want;
        return VELO_OK;
    }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; cap = 0; }
};

// a pinned staging buffer and the device buffer it is copied to or from, reserved together, each by its own growth rule; where the
// parts of such a buffer lie is a StageLayout's to say (velo_stage_layout.h)
struct StagePair {
    PinBuf<> h;
    DevBuf<unsigned char> d;
    int reserve(size_t bytes) { VELO_TRY(h.reserve(bytes)); return d.reserve(bytes); }
};

// One owner for every runtime handle that is not memory with a size: move-only, null by default, destroyed with its holder.  It converts to
// the raw handle, so launch, record and wait sites read as they would with a bare one; put() is where a create call writes a fresh handle.
template <typename H, auto Destroy>
struct Owned {
    H h = nullptr;
    Owned() = default;
    explicit Owned(H x) : h(x) {}
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    Owned(Owned&& o) noexcept : h(o.h) { o.h = nullptr; }
    Owned& operator=(Owned&& o) noexcept { if (this != &o) { reset(o.h); o.h = nullptr; } return *this; }
    ~Owned() { reset(); }
    void reset(H x = nullptr) { if (h) (void)Destroy(h); h = x; }
    H* put() { reset(); return &h; }
    H get() const { return h; }
    operator H() const { return h; }
};
using Stream = Owned<hipStream_t, hipStreamDestroy>;
using GraphExec = Owned<hipGraphExec_t, hipGraphExecDestroy>;
using IpcMap = Owned<void*, hipIpcCloseMemHandle>;                      // a peer's allocation mapped into this process
template <typename T> using DevRaw = Owned<T*, hipFree>;                // a device allocation DevBuf does not make (the fine-grained slabs)
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    int ensure(unsigned flags = hipEventDisableTiming) {                // created on first use; one compare from then on
        if (!h) HIP_TRY(hipEventCreateWithFlags(&h, flags));
        return VELO_OK;
    }
    // the host may write a staging buffer again once the event recorded behind its last upload has passed; the first use creates the event
    int wait_or_create() {
        if (h) HIP_TRY(hipEventSynchronize(h));
        else HIP_TRY(hipEventCreateWithFlags(&h, hipEventDisableTiming));
        return VELO_OK;
    }
};
// start / stop events of a timed launch, from a pool that grows by one pair when all are in use (pairs, once made, are reused)
struct EventPair { Event a, b; };
template <typename P>
P* next_event_pair(std::vector<P>& pool, int* used) {
    if (*used >= (int)pool.size()) {
        P p;
        if (p.a.ensure(hipEventDefault) != VELO_OK || p.b.ensure(hipEventDefault) != VELO_OK) return nullptr;
        pool.push_back(std::move(p));
    }
    return &pool[(size_t)(*used)++];
}

// double-buffered upload staging: two pinned slots used alternately, so that an upload waits only for the one before the previous one
struct PinStage {
    PinBuf<> buf[2];
    Event ev[2];
    int k = 0;
    int acquire(size_t bytes, unsigned char** p) {
        VELO_TRY(ev[k].wait_or_create());
        VELO_TRY(buf[k].reserve(bytes));
        *p = buf[k].p;
        return VELO_OK;
    }
    int sent(hipStream_t stream) {       // behind the copy out of the slot acquire() gave
        HIP_TRY(hipEventRecord(ev[k], stream));
        k ^= 1;
        return VELO_OK;
    }
};

struct Grid {
    GridDesc d{};
    double gate = 0.0;          // squared-distance gate the cell size was derived from
    double h = 0.0;             // cell size
    DevBuf<int> cell_start;     // 3 + ncells + 1: the table starts at element 3, so that table + 1 -- what the one-pass scan and the scatter work on -- is 16-byte aligned
    int* table() const { return cell_start.p + 3; }
    DevBuf<float4> sorted;      // cell-sorted copy {x,y,z,bits(gidx)} (+ kGridPad sentinels)
    DevBuf<int> sring;
    // compressed table (VELO_GRID_COMPRESS=1 in the diagnostics build, see GridView and build_grid): occupancy bits + occupied cells before every word;
    // cell_start then holds the start of every OCCUPIED cell (at most n + 1 entries)
    DevBuf<unsigned long long> wmask;
    DevBuf<int> wprefix;
    int wpr = 0;                // words per grid row; 0 = dense table
    size_t table_len() const { return wpr > 0 ? (size_t)n_points_cap + 1 : (size_t)d.ncells + 1; }   // entries of table() in use
    size_t n_words() const { return (size_t)wpr * (size_t)d.ny * (size_t)d.nz; }
    int n_points_cap = 0;       // compressed: the target's point count when the table was built
    bool built = false;
    void view(GridView* V) const {
        V->d = d; V->cell_start = table(); V->sorted = sorted.p; V->sring = sring.p;
        V->wmask = wpr > 0 ? wmask.p : nullptr; V->wprefix = wpr > 0 ? wprefix.p : nullptr; V->wpr = wpr;
    }
};

struct HostStatus {   // pinned; one D2H copy per LM chunk
    LMState s;
};

void default_params(velo_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->icp_skip = 200; p->f2f_iterations = 2; p->icp_iterations = 3;          // kitti.h:8-10
    p->enable_icp = 1; p->enable_2d2d = 1; p->enable_3d2d = 1;                  // main.cpp:43-45,404
    p->max_num_iterations = 50; p->max_consecutive_invalid_steps = 5;
    p->weight_3D2D = 10; p->weight_2D2D = 500; p->weight_3DPD = 1;              // kitti.h:20-22
    p->loss_thresh_3D2D = 0.01; p->loss_thresh_2D2D = 0.00002;                  // kitti.h:23-24
    p->loss_thresh_3DPD = 0.1; p->loss_thresh_3D3D = 0.04;                      // kitti.h:25-26
    p->outlier_reject = 5.0; p->correspondence_thresh_icp = 0.5;                // kitti.h:30-31
    p->icp_norm_condition = 1e-5;                                               // kitti.h:32
    p->function_tolerance = 1e-6; p->gradient_tolerance = 1e-10; p->parameter_tolerance = 1e-8;
    p->initial_trust_region_radius = 1e4; p->max_trust_region_radius = 1e16;
    p->min_trust_region_radius = 1e-32; p->min_relative_decrease = 1e-3;
    p->min_lm_diagonal = 1e-6; p->max_lm_diagonal = 1e32;
}

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Environment surface.  The PRODUCT library reads five documented, result-preserving knobs (include/velo_hip.h, "environment"):
// VELO_CHAIN, VELO_CHAIN_MARGIN, VELO_BATCH_GROUPS, VELO_BATCH_LOCKSTEP, VELO_SPIN.  Every other switch -- kernel variants, grid
// shapes, A/B paths, diagnostics -- exists only in the tools' build (-DVELO_DIAGNOSTICS, libvelo_hip_diag.so): a drop-in
// frameToFrame whose kernel selection followed leaked environment variables would not be a product surface (the reference's knobs
// are compile-time constants, kitti.h:3-35).  The parity tests that sweep variants load the diagnostics library.
inline const char* dev_env(const char* name) {
#ifdef VELO_DIAGNOSTICS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

}  // namespace

// What set_target builds: the target cloud and its search index.  Held through a shared_ptr: contexts that register different
// scans against the same map (scan-to-map batches) share ONE copy -- 110 MB for a 2M-point map instead of one per context, one index
// build instead of one per context.  Read-only once built; a context that loads a new target while others still hold this one
// starts a fresh TargetData instead of overwriting it.
struct TargetData {
    int n_tgt = 0, n_tgt_rings = 0;
    int tgt_first_ring = 0, tgt_first_point = 0;   // target-sharded mode: global ids of the first local ring / point
    DevBuf<float4> tgt;
    DevBuf<float4> tgt_pad;              // ring-major copy with a wrap-around sentinel on either side of every ring (pad_rings_kernel)
    DevBuf<int> tgt_off, tgt_ring_of, tgt_cell_of;
    std::vector<int> h_tgt_off;
    std::vector<Grid> grids;             // one per distinct gate among iter = 1..f2f_iterations
    float bbox[6] = {0, 0, 0, 0, 0, 0};
    DevBuf<unsigned long long> dimg;     // direction image (kDimgW x kDimgH nearest-point keys): where the seeds of a round without good predecessors come from
    bool dimg_built = false;
};

// one image slot of a context (velo_set_images): every camera's pyramid, camera-major, cam_pix elements apart
struct LkSlot {
    DevBuf<unsigned char> pix;           // padded levels, uint8
    DevBuf<int> der;                     // padded Scharr derivatives, dx | dy << 16
    LkPyr pyr{};
    long long cam_pix = 0;
    int n_cams = 0, w = 0, h = 0;
    bool valid = false;
};

struct LmStore;   // the resident landmark store (velo_api_landmarks.inl)
struct FrStore;   // the resident keypoint frames (velo_api_frames.inl)
struct GraphStore;   // the resident pose graph (velo_api_graph.inl)

struct velo_ctx {
    int device = 0;
    // Members go in reverse order of declaration: the context's own stream is declared before every other handle and buffer, so it is
    // the last of them to be destroyed -- whatever is freed before it is freed while the stream it was used on still exists.
    Stream own_stream;
    hipStream_t stream = nullptr;        // where this context's work is enqueued: own_stream, except while the leader of a lock-step group lends its own
    velo_params P;
    int timing = 0;                      // 0 off, 1 association launches (velo_summary::assoc_kernel_ms), 2 every instrumented launch by kernel name
    int assoc_variant = -1;              // VELO_ASSOC_VARIANT: -1 = default (tube kernel 5); 0 = per-lane reference kernel; 1/2/4/8 = waves per group
                                         // of the box walk; 5 = tube kernel
    int cluster_w = 6;                   // cluster radius of the box kernels, in cells of the default grid (VELO_CLUSTER_W)
    bool cluster_w_set = false;          // the tube kernel keeps one cluster per group unless VELO_CLUSTER_W is given
    int persistent_wgs = 2048;           // workgroups of the persistent association kernel (VELO_PERSISTENT_WGS)
    int xcd_map = 0;                     // box kernels: XCD-contiguous group mapping (VELO_XCD_MAP=1): measured slower
    int tube_map = -1;                   // tube kernel (VELO_TUBE_MAP): -1 = groups in ring order (default); 1 = XCD k works on the k-th eighth of
                                         // every ring (a wedge of the scene): L2 hit rate 57 % -> 73 %, yet 8 % SLOWER (the kernel is bound by VALU
                                         // issue and per-group latency chains, not by L2 misses); 0 = ring order through the same table
                                         // (dense bottom rings all land on one XCD); round-robin placement balances better
    int debug_skip = 0;                  // timing experiments only (VELO_DEBUG_SKIP): results are wrong when non-zero

    // target (frame2): cloud + search index, shareable between contexts (velo_share_target: many scans against one map)
    std::shared_ptr<TargetData> T = std::make_shared<TargetData>();
    DevBuf<int> vis_counts;                       // chain mode: [f2f iteration][blocks, residuals] selected by the device-side gate
    DevBuf<int> scan_tiles, cursor, scan_total;   // scratch of an index build / of the segmenter's scans
    struct { const char* dsrc = nullptr; int64_t stride = 0; bool on = false; } src_raw;   // set_source: the records the fused ingest launch still has to read (source_finalize)
    bool src_bbox_valid = false;         // h_int[16..21] hold the bounding-box keys of the source cloud (source_ingest; on the host once src_bbox_ev has passed)
    Event src_bbox_ev;                   // recorded behind the keys' copy: a promotion waits on it (a no-op after any completed call) before it trusts them
    bool target_early = false;           // promote_begin already sized and enqueued the index (box known): target_finalize_end has nothing to wait for
    int lb_zeroed = 0;                            // status words of the one-pass scan that target_ingest_kernel cleared for the next build (0: build_grid clears them)
    bool batch_load = false;                      // set while velo_register_batch loads this context's scans for a batch of two or more (see build_grid)
    DevBuf<unsigned long long> lb_status;         // one-pass scan: tile status words + ticket
    DevBuf<unsigned> bbox_keys;
    bool have_target = false;

    // source (frame1)
    int n_src = 0, n_src_rings = 0, n_q = 0;
    DevBuf<float4> src;
    DevBuf<int> src_off, q_off, q_src;
    std::vector<int> h_src_off, h_q_off;
    int src_skip = 0;                    // icp_skip the query list was built with
    DevBuf<float4> qpts_buf;             // query points by query index when icp_skip > 1 (with icp_skip == 1 the source cloud is the list)
    const float4* qpts = nullptr;
    DevBuf<float4> prev_a;               // tube kernel warm start: last round's two winners per query with their coordinates (index -1 = none; [0, nq) best, [nq, 2 nq) second),
    DevBuf<int2> prev_r;                 // and their rings; reset with every new source / target
    bool prev_ready = false;             // the seed arrays hold n_q initialised entries for the current source and target
    bool prev_filled = false;            // ... they hold "no previous winner" everywhere already (written by the launch that loaded the source: advance_ingest_kernel)
    int prev_filled_nq = -1;             // ... for this many queries
    int warm_start = 1;                  // VELO_WARM_START=0 turns the seeds off (A/B; results are identical either way)
    int assoc_lds_pad = 0;               // bytes of unused dynamic LDS per association workgroup -- caps the association kernel's workgroups per
                                         // CU so that LM workgroups of other pairs in flight find room at once.  Set by the lock-step batch
                                         // driver when several groups share the chip (kAssocPadShared); VELO_ASSOC_LDS_PAD (diagnostics build) fixes it
    bool assoc_lds_pad_fixed = false;
    int lm_persist = 0;                  // VELO_LM_PERSIST=1 (diagnostics build): lock-step groups in chain mode run a whole solve as ONE launch
                                         // (lm_solve_persist_batch_kernel).  Exact (bit-identical), measured, NOT a gain: an iteration inside the launch
                                         // takes 28 us alone (six agent-scope hand-overs between workgroups) against 19 us for a launch; 8 pairs in
                                         // flight 2,742 vs 3,376 pairs/s -- the waiting workgroups hold registers the association kernels want
    int lm_persist_wgs = 0;              // workgroups per context of that launch (0 = one per virtual block); VELO_LM_PERSIST_WGS (diagnostics build)
    DevBuf<SolveCtl> solve_ctl;          // its per-context control blocks (owned by the first context of a group; zero between launches)
    DevBuf<AgCtl> ag_ctl;                // all-gather solve (lm_solve_ag_batch_kernel, lm_persist == 2): epoch, abort word and flags per context of a group
    int lm_slim = -1;                    // the lean launch's 126-VGPR form (rows one by one): -1 = for groups on a density-shrunk grid; VELO_LM_SLIM (diagnostics build) forces 0 / 1
    int lm_lean = -1;                    // lean fused LM kernel in lock-step groups: -1 = when several groups share the chip; VELO_LM_LEAN (diagnostics build) forces 0 / 1
    // chain mode: a whole frame_to_frame as ONE chain of launches (pose scalars of the next round and the solve summaries stay on the device)
    int patch_order = 1;                 // query list in patch order (VELO_PATCH_ORDER=0: the reference's ring order)
    bool q_patch = false;                // the current list is in patch order
    int patch_rings = kPatchRingsDefault, patch_len = kPatchLenDefault;   // VELO_PATCH_SHAPE=rings,points
    bool ring_order_forced = false;      // this context exchanges per-query records with others (target-sharded workflow): the list stays in the reference's order
    int direct_max = 12288;              // sparse rounds (icp_skip >= direct_skip) of at most this many queries search one wave per query
    int direct_skip = 4;                 // (VELO_ASSOC_DIRECT_MAX, 0 = never; VELO_ASSOC_DIRECT_SKIP)
    // Density-shrunk grids (scan-to-map), single calls: a group whose phase-1 boxes span more than dense_rows grid rows -- queries strung
    // along a wall that thirty scans have sampled: 12,000-17,000 staged candidates -- is searched query by query as a whole, provided at
    // most dense_far of its members have a bound beyond four cells (see assoc_search_v5_body).  Measured on the 2M-point map, us per round
    // of a call: 450 / 402 / 305 / 231 / 230 / 137 -> 435 / 396 / 215 / 149 / 165 / 102, single registration 2.56 -> 2.35 ms.  A launch
    // ends with its slowest group, and these are the slowest; with 8 pairs in flight other groups' kernels fill that tail anyway and the
    // step does not move (1,242 vs 1,235 pairs/s), so lock-step batches keep the tile path (dense_batch).  VELO_DENSE_ROWS / VELO_DENSE_FAR /
    // VELO_DENSE_BATCH (diagnostics build) override.
    int dense_rows = 384, dense_far = 2, dense_batch = 0;
    int asker_queue = 1;                 // shrunk grid: asking queries go to assoc_asker_kernel (VELO_ASKER_QUEUE=0: searched inside their group's workgroup)
    int ask_map = 0;                     // VELO_ASK_MAP: which list entries a wave of the asker kernel takes (0 strided, 1 contiguous + XCD-chunked)
    DevBuf<int> ask_count, ask_list;
    DevBuf<unsigned long long> ask_keys;
    DevBuf<int2> ask_rings;
    int ask_idx = 0;
    bool ask_clean[2] = {false, false};
    bool lm_trace_vis_off = false;       // VELO_LM_MERGED_VIS=0: calls with visual blocks keep sweep + visual sweep + step as three launches (A/B)
    bool want_stats = false;             // velo_set_residual_stats
    DevBuf<double> stat_vals, stat_part;
    DevBuf<signed char> stat_types;
    DevBuf<int> stat_hist;
    DevBuf<StatWork> stat_work;
    DevBuf<velo_residual_stats> stat_out;
    int assoc_lane = 0;                  // VELO_ASSOC_LANE=1: rounds that start from seeds use the lane kernel (A/B; slower, see assoc_lane_body)
    int seed_rounds = 0;                 // association rounds since the seeds were last cleared
    int xcd_chunks = 0;                  // VELO_XCD_CHUNKS=1 (diagnostics build): XCD k searches the k-th eighth of the query list (see assoc_search_v5_body)
    int cu_mask_mode = 0;                // VELO_CU_MASK=1|2 (diagnostics build): this context's stream is confined to a quarter of the CUs (1: bits 64 q .. 64 q + 63,
                                         // 2: the bits i with (i % 8) / 2 == q), q = (creation order / 2) % 4 -- the experiment of giving every lock-step group its own CUs
    int dimg_seeds = 0;                  // VELO_DIMG_SEEDS=1 (diagnostics build): seeds of iteration-1 rounds from the target's direction image (seed_kernel).
                                         // Measured, exact, NOT a gain: C2 rounds 95 / 80 / 78 -> 90 / 86 / 85 us (the cold round's cost is the true
                                         // second-ring distance of the far queries, not poor seeds; the seed launch costs 7 us), 8 pairs in flight
                                         // 3,305 -> 3,354 pairs/s (noise); 2M-point map 1,233 -> 1,050 (0.35-degree buckets are 4 cells wide there)
    int chain_calls = 0;                 // calls that went down the chain
    int chain_margin = 2;                // LM launches enqueued per solve beyond the previous call's count (VELO_CHAIN_MARGIN)
    int chain_misses = 0;                // calls whose chain was too short and were repeated by the host-driven path
    int chain = 1;                       // VELO_CHAIN=0: host round trip after every solve (A/B; identical results)
    DevBuf<PoseRecord> pose_rec;
    DevBuf<SolveLog> solve_log;
    DevBuf<int> chain_fail;
    PinBuf<SolveLog> h_log;              // pinned: VELO_MAX_SOLVES logs + the failure flag behind them
    int lm_fused = 1;                    // VELO_LM_FUSED=0: the lock-step batch driver launches sweep and LM step separately (A/B, identical results)
    int lm_vis_merged = 1;               // chained batch solves with visual blocks run them INSIDE the fused sweep + step launch (extra workgroups, eval_step_batch_(lean_)vis_kernel);
                                         // VELO_LM_VIS_MERGED=0: a launch of their own ahead of it (A/B, identical results)
    int lm_iter = 0;                     // VELO_LM_ITER=1: chained batch solves launch the lean one-launch iteration (every workgroup advances the state itself) instead of the fused sweep + step (A/B, identical results; measured slower: 3,204 vs 3,418 pairs/s)
    int lm_merged = 1;                   // VELO_LM_MERGED=0: sweep and LM step as two launches per iteration also where one would do (A/B, identical results)
    int small_solve = 1;                 // VELO_SMALL_SOLVE=0: small problems go through the launch-per-iteration path too (A/B, identical results)
    int asker_rows = -1;                 // tube kernel (VELO_ASKER_ROWS): phase 2 goes query by query when the asking queries' boxes have more
                                         // rows than this in total.  -1 = by target density: never on a regular scan (120k points: the tile pass
                                         // is 62 vs 105-115 us), always when the grid had to be density-shrunk (2M-point map: 244 vs 420 us)
    DevBuf<FunctorRec> fn_in;            // velo_evaluate_functors: the records of one call
    DevBuf<int> group_perm;              // workgroup -> 64-query group, XCD-aware (see build_group_perm)
    int perm_qb = -1, perm_qe = -1, perm_nq = -1, perm_mode = -1;
    bool have_source = false;

    DevBuf<char> staging;                // raw host clouds land here before packing
    // velo_hint_next_source: the NEXT frame's raw host cloud is uploaded on a copy stream of its own while this frame's chain of launches runs
    // (main.cpp:216 loads a scan per frame): two landing buffers, so the upload for frame k + 2 never touches what frame k + 1's ingest reads
    struct Prefetch {
        const void* host = nullptr; size_t bytes = 0; bool hinted = false, ready = false; int buf = 0;
        DevBuf<char> land[2]; Stream stream; Event ev;
        PinBuf<char> pin[2]; bool in_pin = false;   // the announced cloud in page-locked memory of the library's own (see prefetch_issue)
    } pf;
    // velo_hint_next_frame: the NEXT frame of a drive -- promote the scan held as source, load the announced scan as the new source, build the
    // index -- is enqueued BEHIND the current registration's chain of launches, before the calling thread waits for it: the loads of frame
    // k + 1 run while the host wakes up, reads frame k's results and hands the pose over (the step boundary, where every queue used to
    // drain).  The old target's cloud is kept until the call is known to be good: a call that has to be repeated host-driven gets its pair back.
    struct NextFrame {
        enum State { NONE = 0, LOADED = 2, CONSUMED = 3 };
        int state = NONE;                   // of the frame loaded ahead: LOADED until the job that brings it arrives, CONSUMED while that job runs
        velo_scan_ref ref{};                // ... and its descriptor
        bool hint_valid = false;            // an announcement waiting for the end of the current call's enqueue (it may arrive while `state` is LOADED:
        velo_scan_ref hint{};               //  the caller announces frame k + 1 before the job of frame k, loaded ahead one call ago, has been handed over)
        DevBuf<float4> undo_cloud; std::vector<int> undo_off; int undo_n = 0, undo_rings = 0;   // the old target's cloud: its BUFFER, rotated out (no copy)
        DevBuf<unsigned> keys; int parity = 0;   // group-batched loads (AdvJob): the source's bounding-box keys in two slots, used alternately
        Event call_done;                    // behind the call's last read-back copy: what the calling thread waits for when more has been enqueued behind it
    } nf;
    double last_chain_us = 0.0;          // the previous chained lock-step call this context led: enqueue -> results in (sizes the stagger of the groups' starts)
    AdvJob* adv = nullptr;               // set while a group's loads are being COLLECTED (preload_group): target_ingest / build_grid / source_ingest fill it instead of launching
    DevBuf<int> seg_flag, seg_excl, seg_ring, seg_off;   // device-side ring segmentation (velo_set_scan_velodyne)

    // correspondence table
    DevBuf<float4> cp, cn, cv0, aux1;
    DevBuf<int4> aux0;
    DevBuf<int> n_valid;                 // two counters used alternately: the association kernel of one round clears the counter of
    int nv_idx = 0;                      // the next, so no fill launch (and no 18 us launch gap behind it) per round
    bool nv_clean[2] = {false, false};   // counter is zero on the stream's timeline
    DevBuf<unsigned long long> dbg, wg_times;
    int wg_times_n = 0;
    DevBuf<AssocItem> items;             // work queue of the pipelined association
    DevBuf<int> item_counters;
    DevBuf<float4> qpos;
    DevBuf<PartialRec> partials_rec, partials_all;   // target-sharded mode: my records for all queries / every rank's records for my queries
    bool have_partials = false;
    int last_partial_iter = 1;           // gate of the last partial association (the merge needs its key_inf)
    bool target_sharded = false;
    bool have_corr = false;
    int last_n_valid = 0;

    // visual
    int n_matches = 0;
    DevBuf<VisualMatch> vm;
    DevBuf<unsigned char> vflags;
    std::vector<velo_match> h_matches;
    std::vector<unsigned char> h_vflags;
    bool vflags_valid = false;
    int vis_frame1 = -1;                 // velo_build_matches[_desc] made the visual set from this frame of the frame store (-1: somebody else did) ...
    uint64_t vis_gen[8] = {};            // ... when its cameras' entries had these stamps (velo_frames_prune asks)

    // LM
    DevBuf<LMState> state;
    DevBuf<LMEvalPoint> eval_pt;         // where the next sweep evaluates: written by lm_begin / the LM step, read by the sweep workgroups
    DevBuf<double> partials, reduced, xdev;
    DevBuf<int> ticket;
    DevBuf<int> batch_tickets;                    // fused sweep + step of a lock-step group: one ticket counter per context (0 at launch boundaries)
    DevBuf<unsigned long long> lm_trace;  // diagnostics build, VELO_LM_TRACE=1: stage stamps of the LM chain (tools/lm_trace.py)
    bool lm_trace_on = false;
    int lm_trace_idx = 0;                 // launches of the current solve so far
    // captured LM chunks (single GPU): key = iterations per chunk; rebuilt when anything baked into the nodes changes
    GraphExec chunk_graph[2];
    int chunk_graph_iters[2] = {0, 0};
    std::vector<unsigned char> chunk_graph_sig[2];   // bytes of everything baked into the nodes
    bool use_graphs = false;             // LM chunks as hipGraphs (VELO_GRAPHS=1): measured no gain, replay overhead ~ launches saved
    int pred_evals[VELO_MAX_SOLVES];     // evaluations each solve of the previous frame_to_frame needed (chunk sizing)
    int eval_hist[VELO_MAX_SOLVES][4];   // ... and of the last four calls: how far a solve's count moves decides the chain's margin
    int eval_hist_n[VELO_MAX_SOLVES];
    bool chain_margin_fixed = false;     // VELO_CHAIN_MARGIN given: that margin, always
    PinBuf<HostStatus> h_status;         // pinned
    PinBuf<double> h_x;                  // pinned, 64 doubles
    PinBuf<int> h_int;                   // pinned scratch: [0] counters, [8..13] target box keys, [16..21] source box keys
    // pinned staging for the small host tables a load sends to the device (source ring offsets, query offsets): the copy is asynchronous
    // and the slot's event says when the host may write the slot again -- no stream synchronisation at the end of a load
    struct PinSlot { PinBuf<int> buf; Event ev; bool pending = false; };
    PinSlot pin[4];                               // 0: source ring offsets (+ query offsets), 1: query offsets, 2: target ring offsets + bounding-box keys,
                                                  // 3: the visual matches on their way to the device (set_visual_impl without a wait)
    DevBuf<int> row_off_vis, row_off_icp;
    DevBuf<double> rows_r, rows_J;

    // camera projection of a scan + keypoint depth association
    DevBuf<float4> pstack, vstack, kp_point, kp_out;
    DevBuf<float2> kps;
    DevBuf<int> proj_off, ring_cnt, kp_flag, kp_excl, kp_has;
    std::vector<int> h_proj_off, h_ring_cnt;   // offsets of the projected cloud (copied: the cloud may be replaced later)
    int proj_rings = 0, proj_points = 0, proj_of_target = 0;
    bool have_projection = false;

    // batched landmark triangulation
    DevBuf<TriFrame> tri_frames;
    DevBuf<double> tri_cam_t;
    DevBuf<velo_tri_obs> tri_obs;
    DevBuf<int> tri_off;
    DevBuf<float> tri_pts;
    DevBuf<unsigned char> tri_init;
    DevBuf<velo_tri_result> tri_res;
    int tri_variant = 1;                 // 1 = one wave per landmark (default), 0 = one thread per landmark (VELO_TRI_VARIANT)

    // descriptor matching (velo_match_descriptors): buffers of its own, which no registration reads or writes
    StagePair md_in;                     // one staged upload: job table | the distinct descriptor rows (64 bytes each)
    DevBuf<unsigned> md_keys;            // [sum n_query] nearest-row keys | [n_jobs] min_dist
    DevBuf<int> md_out;                  // train_idx | distance | pairs (per job from its first query) | {min_dist, n_kept} per job
    PinBuf<int> h_md_out;                // pinned landing of md_out
    int match_variant = 1;               // 1 = int8 MFMA (product), 0 = XOR + popcount (VELO_MATCH_VARIANT, diagnostics build only)

    // resident camera images and Lucas-Kanade tracking (velo_set_images / velo_track_features): buffers of their own, which no
    // registration reads or writes
    LkSlot lk_slot[2];                   // current = lk_slot[lk_cur], previous = the other (velo_set_images rotates them)
    int lk_cur = 0;
    StagePair lk_raw;                    // unit table | level tables | the frame's raw images, one upload
    Event lk_upload_ev;                  // lk_raw.h may be rewritten once this has passed
    StagePair lk_in;                     // job table | level tables | points
    StagePair lk_out;                    // next_xy | status | kept
    DevBuf<unsigned long long> lk_diag;  // diagnostics build: iterations / entries per level (velo_diag_track_counters)
    bool lk_diag_init = false;

    // corner detection on the current images (velo_detect_features): buffers of its own, which nothing else reads or writes
    DevBuf<float> gf_eig;                // units x (h x w): the minimum-eigenvalue map
    DevBuf<unsigned char> gf_state;      // units x padded state map (velo_detect_kernels.h)
    DevBuf<unsigned> gf_cand;            // units x (h x w) candidate indices | units x (h x w) undecided at the finish
    DevBuf<unsigned long long> gf_keys;  // units x keys_cap accepted keys
    DevBuf<int> gf_hdr;                  // units x kGfHdrStride (a 128-byte line per unit)
    StagePair gf_in;                     // unit table | job table | existing points
    StagePair gf_out;                    // counts | per job xy, response, fresh
    int gf_units = 0;                    // units of the last launch set this context led (velo_diag_detect_counters)
    // the resident landmark store (velo_landmarks_*): created by velo_landmarks_reset, buffers of its own, which no registration reads or writes
    std::shared_ptr<LmStore> lm;
    // the resident keypoint frames (velo_frames_*): created by velo_frames_reset; velo_build_matches writes the visual set (vm, n_matches) from them
    std::shared_ptr<FrStore> fr;
    // the resident pose graph (velo_graph_*): created by velo_graph_reset; nodes, edges and the solver's work buffers, which nothing else reads or writes
    std::shared_ptr<GraphStore> graph;
    // front-end calls over several contexts (fb_gather / fb_release below): the FIRST context of a call lends its stream, staging and scratch buffers
    Event fb_here_ev;                    // "everything enqueued on this context's stream so far": the lending stream waits for it
    Event fb_done_ev;                    // recorded on the lending stream after an asynchronous batch call: the other streams wait for it

    // lock-step batch driver (velo_frame_to_frame_batch): scratch owned by the FIRST context of a batch
    DevBuf<LMBatchItem> batch_items;
    DevBuf<PoseRecord> batch_pose;       // chain mode of the lock-step driver: per-context records, logs, failure flags
    DevBuf<SolveLog> batch_logs;
    DevBuf<int> batch_fail;
    DevBuf<LMState> batch_states;
    DevBuf<double> batch_x;
    PinBuf<> h_batch;                    // pinned: items, x, states
    int batch_lockstep = 1;              // VELO_BATCH_LOCKSTEP=0: one host thread per context instead (A/B)

    // sharding / comm
    int shard_rank = 0, shard_world = 1;
    ncclComm_t comm = nullptr;
    // peer-slab all-reduce (velo_comm_peer_export / _attach): my slab, the peers' mappings, my sequence counter and error word
    DevRaw<PeerSlab> peer_slab;
    bool peer_on = false;
    PeerComm peer{};
    IpcMap peer_mapped[kMaxPeers];
    DevBuf<unsigned long long> peer_seq;
    DevBuf<unsigned long long> peer_kseq;           // counter of the launch-count agreements (peer_agree_kernel)
    PinBuf<int> h_agree;                            // pinned: the agreed launch counts of a chained peer call
    std::vector<DevRaw<PeerSlab>> peer_retired;     // slabs of earlier exports: a peer's timed-out call may still store into them; freed with the context
    DevBuf<int> peer_err;
    DevRaw<PartialRec> peer_area;        // my receive area of the record exchange (fine-grained, exported)
    int peer_area_queries = 0;           // max_queries it was sized for
    IpcMap peer_area_mapped[kMaxPeers];
    PeerRecs peer_recs{};
    bool peer_recs_on = false;
    unsigned long long peer_xseq = 0;    // exchanges so far (all ranks count alike)

    Event ev0, ev1;
    std::vector<EventPair> assoc_events;   // reused pool
    std::vector<std::pair<const char*, uint64_t>> assoc_event_info;  // kernel name + algorithmic bytes of the launch behind each pair
    int assoc_events_used = 0;
    // velo_set_timing(ctx, 2): every instrumented launch (association, LM, index build) is bracketed by the start / stop events of
    // hipExtLaunchKernelGGL; a call's brackets are read after its final synchronisation and added up per kernel name (velo_get_kernel_times)
    struct TimedLaunch : EventPair { const char* name = nullptr; uint64_t bytes = 0; };
    std::vector<TimedLaunch> klog;
    int klog_used = 0;
    struct KernelAcc { const char* name; double ms; int64_t launches, sampled; uint64_t bytes; };   // ms: of the `sampled` bracketed launches
    int timing_every = 8;                    // level 2 brackets every n-th launch of a kernel name (a bracket costs ~5 us of queue time); level 3: every launch
    std::vector<KernelAcc> kacc;
    const char* lm_kernel_name = nullptr;    // the LM kernel the last call launched (its evaluations' algorithmic bytes are known only afterwards)
    const char* lm_round_name[VELO_MAX_SOLVES] = {};   // ... per solve of a chained call: rounds may take different kernels (small solve / sweep + step)
    // a chained call that misses is repeated host-driven: what the abandoned chain logged (counted launches, brackets) is dropped with it
    struct TimingMark { std::vector<KernelAcc> kacc; int klog_used = 0, assoc_events_used = 0; };
    void timing_mark(TimingMark* m) const { if (timing >= 2) { m->kacc = kacc; m->klog_used = klog_used; m->assoc_events_used = assoc_events_used; } }
    void timing_rewind(const TimingMark& m) { if (timing >= 2) { kacc = m.kacc; klog_used = m.klog_used; assoc_events_used = m.assoc_events_used; } }
};

// ---- what the entry points over a LIST of contexts share (images, tracking, detection, the landmark and frame stores, the scan map):
// the checks of the list, the hand-over between the contexts' streams, and the range checks of frame and camera indices ------------------
namespace {
constexpr int kFbMaxCtx = 256;             // contexts per call
constexpr int kLmMaxFrame = 1 << 22;       // frame indices of the landmark store, the frame store, BA and the pose graph

// the checks of the context list that read no context
int fb_check_list(velo_ctx** ctxs, int n_ctx) {
    if (!ctxs) return fail(VELO_ERR_INVALID, "null context list");
    if (n_ctx < 1 || n_ctx > kFbMaxCtx) return fail(VELO_ERR_INVALID, "%d contexts; 1..%d", n_ctx, kFbMaxCtx);
    for (int i = 0; i < n_ctx; i++) {
        if (!ctxs[i]) return fail(VELO_ERR_INVALID, "context %d is null", i);
        for (int j = 0; j < i; j++) if (ctxs[j] == ctxs[i]) return fail(VELO_ERR_INVALID, "batch entries %d and %d are the same context", j, i);
    }
    return VELO_OK;
}

int fb_check_devices(velo_ctx** ctxs, int n_ctx) {
    for (int i = 1; i < n_ctx; i++)
        if (ctxs[i]->device != ctxs[0]->device)
            return fail(VELO_ERR_INVALID, "contexts on different devices: entry %d is on device %d, entry 0 on device %d", i, ctxs[i]->device, ctxs[0]->device);
    return VELO_OK;
}

// job_ctx of the batch entries; null (the single-context entries pass it): every job runs on context 0
int fb_check_job_ctx(const int32_t* job_ctx, int n_jobs, int n_ctx) {
    if (!job_ctx) return VELO_OK;
    for (int j = 0; j < n_jobs; j++)
        if (job_ctx[j] < 0 || job_ctx[j] >= n_ctx) return fail(VELO_ERR_INVALID, "job %d: context index %d; 0..%d", j, job_ctx[j], n_ctx - 1);
    return VELO_OK;
}
inline int fb_ctx_of(const int32_t* job_ctx, int j) { return job_ctx ? job_ctx[j] : 0; }

// the lending stream runs after everything already enqueued on the stream of every other context in `used` (null: all)
int fb_gather(velo_ctx** ctxs, int n_ctx, const std::vector<char>* used) {
    velo_ctx* c0 = ctxs[0];
    for (int i = 1; i < n_ctx; i++) {
        if (used && !(*used)[i]) continue;
        velo_ctx* c = ctxs[i];
        if (c->stream == c0->stream) continue;
        VELO_TRY(c->fb_here_ev.ensure());
        HIP_TRY(hipEventRecord(c->fb_here_ev, c->stream));
        HIP_TRY(hipStreamWaitEvent(c0->stream, c->fb_here_ev, 0));
    }
    return VELO_OK;
}

// whatever is enqueued later on any other context's stream runs after what the lending stream holds now
int fb_release(velo_ctx** ctxs, int n_ctx) {
    velo_ctx* c0 = ctxs[0];
    if (n_ctx < 2) return VELO_OK;
    VELO_TRY(c0->fb_done_ev.ensure());
    HIP_TRY(hipEventRecord(c0->fb_done_ev, c0->stream));
    for (int i = 1; i < n_ctx; i++)
        if (ctxs[i]->stream != c0->stream) HIP_TRY(hipStreamWaitEvent(ctxs[i]->stream, c0->fb_done_ev, 0));
    return VELO_OK;
}

// `name` v of [0, n); the message says where the value came from: nothing, "what: " (idx < 0) or "what idx: "
int check_range(const char* name, int v, int n, const char* what, int idx) {
    if (v >= 0 && v < n) return VELO_OK;
    if (!what) return fail(VELO_ERR_INVALID, "%s %d; 0..%d", name, v, n - 1);
    if (idx < 0) return fail(VELO_ERR_INVALID, "%s: %s %d; 0..%d", what, name, v, n - 1);
    return fail(VELO_ERR_INVALID, "%s %d: %s %d; 0..%d", what, idx, name, v, n - 1);
}
inline int check_frame(int frame, const char* what = nullptr, int idx = -1) { return check_range("frame", frame, kLmMaxFrame, what, idx); }
inline int check_cam(int cam, int n_cams, const char* what = nullptr, int idx = -1) { return check_range("camera", cam, n_cams, what, idx); }

}  // namespace
