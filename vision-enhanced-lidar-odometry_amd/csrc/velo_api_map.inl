// velo_api_map.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: the device-resident sliding-window scan map of scan-to-map odometry (velo_map_*); the kernel is in velo_map_kernels.h.
//
// Who knows what: the DEVICE holds every scan of the window as it was registered -- ring-major float4, in its OWN sensor frame -- in one
// arena of points (FrArena over velo_block_list.h: first-fit free list, geometric growth as the only wait); the HOST keeps the directory
// in insertion order: frame, block, point count, ring offsets (empty rings dropped), pose.  A load materialises the window into a
// context's target buffer in the frame the caller names (one launch for every scan of every map of a call) and then runs the ingest
// and the index build velo_set_target runs, on that buffer in place.  A point is rounded to float once, whatever the drive's length;
// a pose is corrected with no point traffic.
// The map has no stream: an insert or a load runs on the named context's stream and leaves an event behind; a load on another stream
// waits for the last insert, an insert that may take a block a load still reads waits for the last load (a drop only returns the block
// to the free list: the insert that takes it is the one that waits).  Like a scan cache, a map takes one call at a time.
struct velo_map {
    int device = 0;
    int max_scans = 0;
    int64_t max_points = 0;
    FrArena<float4, 1> arena;                        // unit: one point; every block starts on a 64-byte line
    struct Scan { int frame = 0; Block blk; int n = 0; std::vector<int> off; double pose[16] = {}; };
    std::vector<Scan> scans;                         // oldest first
    int64_t points = 0, evictions = 0;
    Event ins_ev, load_ev;                           // behind the last insert's copy / the last load's launch
    hipStream_t ins_stream = nullptr, load_stream = nullptr;   // ... and the streams they were recorded on (compared, never used)
    bool ins_any = false, load_any = false;
    PinStage stage;                                  // the unit table on its way to the device (a batch call uses the first map's)
    DevBuf<unsigned char> d_units;
};

namespace {

constexpr size_t kMapFirstArena = 4096 / sizeof(float4);   // points: the arena starts at 4 KB and doubles up to what the window needs
constexpr size_t kMapAlign = 4;                            // points: 64 bytes
constexpr int64_t kMapMaxPoints = (int64_t)1 << 30;

inline size_t map_round(size_t points) { return (points + kMapAlign - 1) / kMapAlign * kMapAlign; }

int map_find(const velo_map* m, int frame) {
    for (size_t k = 0; k < m->scans.size(); k++) if (m->scans[k].frame == frame) return (int)k;
    return -1;
}

int map_check_pose(const double* p, const char* what) {
    if (!p) return fail(VELO_ERR_INVALID, "null %s", what);
    for (int k = 0; k < 16; k++) if (!std::isfinite(p[k])) return fail(VELO_ERR_INVALID, "%s[%d] is not finite", what, k);
    return VELO_OK;
}

// work about to be enqueued on `st` that READS the map's scans runs after the last insert
int map_order_read(velo_map* m, hipStream_t st) {
    if (m->ins_any && m->ins_stream != st) HIP_TRY(hipStreamWaitEvent(st, m->ins_ev, 0));
    return VELO_OK;
}
// ... that may WRITE where a load reads (a block of the free list, the unit table) runs after the last load
int map_order_write(velo_map* m, hipStream_t st) {
    if (m->load_any && m->load_stream != st) HIP_TRY(hipStreamWaitEvent(st, m->load_ev, 0));
    return VELO_OK;
}

// rows 0..2 of a * b, every entry summed left to right in double (tests/scan_map_ref.py states the same)
void map_compose(const double* a, const double* b, double* m12) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 4; j++)
            m12[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j];
}

// velo_map_load[_batch]: entry i makes maps[i] the target of ctxs[i] in the frame ref_inv[16 i ..]
int map_load_run(velo_map** maps, velo_ctx** ctxs, int n, const double* ref_inv) {
    // every argument and every map's state is checked before any context is touched
    if (!maps) return fail(VELO_ERR_INVALID, "null map list");
    VELO_TRY(fb_check_list(ctxs, n));
    if (!ref_inv) return fail(VELO_ERR_INVALID, "null ref_inv");
    for (int k = 0; k < 16 * n; k++) if (!std::isfinite(ref_inv[k])) return fail(VELO_ERR_INVALID, "entry %d: ref_inv[%d] is not finite", k / 16, k % 16);
    int n_units = 0, max_n = 0;
    for (int i = 0; i < n; i++) {
        if (!maps[i]) return fail(VELO_ERR_INVALID, "map %d is null", i);
        if (ctxs[i]->device != maps[i]->device) return fail(VELO_ERR_INVALID, "entry %d: context on device %d, map on device %d", i, ctxs[i]->device, maps[i]->device);
    }
    VELO_TRY(fb_check_devices(ctxs, n));
    for (int i = 0; i < n; i++) {
        const velo_map* m = maps[i];
        if (m->scans.empty()) return fail(VELO_ERR_STATE, "entry %d: the map holds no scan", i);
        if (m->points > (int64_t)INT32_MAX - 4096) return fail(VELO_ERR_STATE, "entry %d: %lld points do not fit a target", i, (long long)m->points);
        n_units += (int)m->scans.size();
        for (const velo_map::Scan& s : m->scans) max_n = std::max(max_n, s.n);
    }
    if (n_units > 65535) return fail(VELO_ERR_INVALID, "%d scans in one call; at most 65535", n_units);
    velo_ctx* c0 = ctxs[0];
    velo_map* m0 = maps[0];
    HIP_TRY(hipSetDevice(c0->device));
    // every context's target: the window's points and the concatenated ring offsets, as velo_set_target takes them
    for (int i = 0; i < n; i++) {
        velo_ctx* c = ctxs[i];
        const velo_map* m = maps[i];
        own_target(c);
        c->have_target = false; c->have_corr = false; c->have_partials = false;
        TargetData& T = *c->T;
        T.tgt_first_ring = 0; T.tgt_first_point = 0;
        T.h_tgt_off.assign(1, 0);
        int at = 0;
        for (const velo_map::Scan& s : m->scans) {
            for (size_t r = 1; r < s.off.size(); r++) T.h_tgt_off.push_back(at + s.off[r]);
            at += s.n;
        }
        T.n_tgt = at; T.n_tgt_rings = (int)T.h_tgt_off.size() - 1;
        VELO_TRY(T.tgt.reserve((size_t)std::max(at, 1)));
    }
    // the unit table: one entry per scan, entry-major, oldest scan first
    const size_t bytes = sizeof(MapUnit) * (size_t)n_units;
    unsigned char* pin = nullptr;
    VELO_TRY(m0->stage.acquire(bytes, &pin));
    VELO_TRY(m0->d_units.reserve(bytes));
    {
        MapUnit* hu = reinterpret_cast<MapUnit*>(pin);
        int u = 0;
        for (int i = 0; i < n; i++) {
            int at = 0;
            for (const velo_map::Scan& s : maps[i]->scans) {
                MapUnit& U = hu[u++];
                U.src = maps[i]->arena.at(s.blk);
                U.dst = ctxs[i]->T->tgt.p + at;
                U.n = s.n; U.pad = 0;
                map_compose(ref_inv + 16 * (size_t)i, s.pose, U.m);
                at += s.n;
            }
        }
    }
    // the lending stream: behind what every context has enqueued (their old targets are still read there), behind the maps' last inserts
    // and -- the table is overwritten -- behind the last load that read it
    hipStream_t st = c0->stream;
    VELO_TRY(fb_gather(ctxs, n, nullptr));
    // EVERY map of the call waits for its own last load on another stream, not only the first one, whose table is rewritten: so the loads
    // of a map form one chain on the device, and load_ev -- recorded below for every map -- stands for all loads before it.  That chain is
    // what lets an insert wait for the LAST load alone before it takes a block an earlier load may still read; do not relax it to maps[0].
    for (int i = 0; i < n; i++) { VELO_TRY(map_order_read(maps[i], st)); VELO_TRY(map_order_write(maps[i], st)); }
    HIP_TRY(hipMemcpyAsync(m0->d_units.p, pin, bytes, hipMemcpyHostToDevice, st));
    VELO_TRY(m0->stage.sent(st));
    const uint64_t total = [&] { uint64_t t = 0; for (int i = 0; i < n; i++) t += (uint64_t)maps[i]->points; return t; }();
    VELO_LAUNCH_T(c0, "map_materialise_kernel", 32ull * total, map_materialise_kernel, dim3((unsigned)cdiv(max_n, kMapTile), (unsigned)n_units), dim3(kMapThreads), 0, st,
                  reinterpret_cast<const MapUnit*>(m0->d_units.p));
    HIP_TRY(hipGetLastError());
    for (int i = 0; i < n; i++) {
        velo_map* m = maps[i];
        VELO_TRY(m->load_ev.ensure());
        HIP_TRY(hipEventRecord(m->load_ev, st));
        m->load_stream = st; m->load_any = true;
    }
    VELO_TRY(fb_release(ctxs, n));
    // ingest and bounding-box request of every context on its own stream, in place on the materialised cloud, before any is waited for
    for (int i = 0; i < n; i++) VELO_TRY(target_ingest(ctxs[i], reinterpret_cast<const float*>(ctxs[i]->T->tgt.p), (int64_t)sizeof(float4), 1));
    for (int i = 0; i < n; i++) VELO_TRY(target_finalize_end(ctxs[i]));
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)

int velo_map_create(velo_map** out, int32_t device, int32_t max_scans, int64_t max_points) {
    if (!out || max_scans < 1 || max_points < 1 || max_points > kMapMaxPoints) return fail(VELO_ERR_INVALID, "bad map arguments");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) return fail(VELO_ERR_NODEVICE, "no HIP device visible: the scan map lives in device memory");
    if (device < 0 || device >= n_dev) return fail(VELO_ERR_INVALID, "device %d out of range (%d visible)", device, n_dev);
    HIP_TRY(hipSetDevice(device));
    std::unique_ptr<velo_map> m(new velo_map());
    m->device = device; m->max_scans = max_scans; m->max_points = max_points;
    VELO_TRY(m->arena.buf.reserve(kMapFirstArena));
    m->arena.list.cap = kMapFirstArena;                 // the buffer holds a little more; the arena reallocates at what was asked for
    *out = m.release();
    return VELO_OK;
}

int velo_map_destroy(velo_map* m) {
    if (!m) return VELO_OK;
    (void)hipSetDevice(m->device);
    if (m->load_any) (void)hipEventSynchronize(m->load_ev);   // nothing reads the arena when it goes
    if (m->ins_any) (void)hipEventSynchronize(m->ins_ev);
    delete m;                                           // members release their memory and their events
    return VELO_OK;
}

int velo_map_insert(velo_map* m, velo_ctx* c, int32_t of_target, int32_t frame, const double pose16[16], int32_t* n_evicted) {
    if (n_evicted) *n_evicted = 0;
    if (!m || !c) return fail(VELO_ERR_INVALID, "null argument");
    VELO_TRY(map_check_pose(pose16, "pose16"));
    if (c->device != m->device) return fail(VELO_ERR_INVALID, "context on device %d, map on device %d", c->device, m->device);
    if (of_target ? !c->have_target : !c->have_source) return fail(VELO_ERR_STATE, "the context holds no %s scan", of_target ? "target" : "source");
    if (of_target && (c->T->tgt_first_ring != 0 || c->T->tgt_first_point != 0)) return fail(VELO_ERR_STATE, "a target shard is not a whole scan");
    if (map_find(m, frame) >= 0) return fail(VELO_ERR_STATE, "frame %d is in the map already: drop it first", frame);
    const int n = of_target ? c->T->n_tgt : c->n_src;
    const std::vector<int>& h_off = of_target ? c->T->h_tgt_off : c->h_src_off;
    if (n <= 0) return fail(VELO_ERR_INVALID, "a scan with no point cannot enter the map");
    if ((int64_t)n > m->max_points) return fail(VELO_ERR_INVALID, "a scan of %d points does not fit a map of at most %lld", n, (long long)m->max_points);
    velo_map::Scan e;
    e.frame = frame; e.n = n;
    e.off.assign(1, 0);
    for (size_t r = 1; r < h_off.size(); r++) if (h_off[r] > h_off[r - 1]) e.off.push_back(h_off[r]);   // a target ring may not be empty
    std::memcpy(e.pose, pose16, sizeof(e.pose));
    // the oldest scans go first: on a copy of the bookkeeping, so that a failure below leaves the window as it was
    size_t gone = 0;
    int64_t left = m->points;
    BlockList list = m->arena.list;
    while (gone < m->scans.size() && ((int)(m->scans.size() - gone) >= m->max_scans || left + n > m->max_points)) {
        list.release(m->scans[gone].blk);
        left -= m->scans[gone].n;
        gone++;
    }
    HIP_TRY(hipSetDevice(m->device));
    hipStream_t st = c->stream;
    VELO_TRY(map_order_read(m, st));                    // (a growth copies what earlier inserts wrote)
    VELO_TRY(map_order_write(m, st));
    const size_t need = map_round((size_t)n);
    if (list.plan(nullptr, need).grow_to > 0 && m->load_any) HIP_TRY(hipEventSynchronize(m->load_ev));   // the old buffer is freed: no load reads it
    BlockList::Plan plan;
    VELO_TRY(m->arena.place(c, &list, nullptr, need, &plan));
    // (the buffer is the larger one from here on, whatever follows: the capacity and the growth count go with it, so that velo_map_info
    //  is right and the next insert does not reallocate again when the copy below fails; blocks and `used` stay as they were until then)
    m->arena.list.cap = list.cap; m->arena.list.reallocs = list.reallocs;
    e.blk = plan.block;
    HIP_TRY(hipMemcpyAsync(m->arena.at(e.blk), of_target ? c->T->tgt.p : c->src.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, st));
    VELO_TRY(m->ins_ev.ensure());
    HIP_TRY(hipEventRecord(m->ins_ev, st));
    m->ins_stream = st; m->ins_any = true;
    list.commit(plan, nullptr);
    m->arena.list = list;
    m->scans.erase(m->scans.begin(), m->scans.begin() + (std::ptrdiff_t)gone);
    m->scans.push_back(std::move(e));
    m->points = left + n;
    m->evictions += (int64_t)gone;
    if (n_evicted) *n_evicted = (int32_t)gone;
    return VELO_OK;
}

int velo_map_set_pose(velo_map* m, int32_t frame, const double pose16[16]) {
    if (!m) return fail(VELO_ERR_INVALID, "null map");
    VELO_TRY(map_check_pose(pose16, "pose16"));
    const int k = map_find(m, frame);
    if (k < 0) return fail(VELO_ERR_STATE, "frame %d is not in the map", frame);
    std::memcpy(m->scans[(size_t)k].pose, pose16, sizeof(double) * 16);
    return VELO_OK;
}

int velo_map_drop(velo_map* m, int32_t frame) {
    if (!m) return fail(VELO_ERR_INVALID, "null map");
    const int k = map_find(m, frame);
    if (k < 0) return fail(VELO_ERR_STATE, "frame %d is not in the map", frame);
    m->arena.list.release(m->scans[(size_t)k].blk);
    m->points -= m->scans[(size_t)k].n;
    m->scans.erase(m->scans.begin() + k);
    return VELO_OK;
}

int velo_map_clear(velo_map* m) {
    if (!m) return fail(VELO_ERR_INVALID, "null map");
    for (const velo_map::Scan& s : m->scans) m->arena.list.release(s.blk);
    m->scans.clear();
    m->points = 0;
    return VELO_OK;
}

int velo_map_frames(const velo_map* m, int32_t* frames_out, int32_t capacity) {
    if (!m) return 0;
    int i = 0;
    for (const velo_map::Scan& s : m->scans) { if (frames_out && i < capacity) frames_out[i] = s.frame; i++; }
    return i;
}

int velo_map_info(const velo_map* m, int64_t* info) {
    if (!m || !info) return fail(VELO_ERR_INVALID, "null argument");
    int64_t rings = 0;
    for (const velo_map::Scan& s : m->scans) rings += (int64_t)s.off.size() - 1;
    info[0] = (int64_t)m->scans.size(); info[1] = m->points; info[2] = rings; info[3] = m->max_scans; info[4] = m->max_points;
    info[5] = m->evictions; info[6] = (int64_t)m->arena.list.cap; info[7] = m->arena.list.reallocs;
    return VELO_OK;
}

int velo_map_get_scan(velo_map* m, int32_t frame, float* xyz, int32_t capacity_points, int32_t* n_points, int32_t* ring_offsets,
                      int32_t capacity_rings, int32_t* n_rings, double pose16[16]) {
    if (n_points) *n_points = 0;
    if (n_rings) *n_rings = 0;
    if (!m) return fail(VELO_ERR_INVALID, "null map");
    const int k = map_find(m, frame);
    if (k < 0) return fail(VELO_ERR_STATE, "frame %d is not in the map", frame);
    const velo_map::Scan& s = m->scans[(size_t)k];
    const int nr = (int)s.off.size() - 1;
    if (n_points) *n_points = s.n;
    if (n_rings) *n_rings = nr;
    if (pose16) std::memcpy(pose16, s.pose, sizeof(double) * 16);
    if (ring_offsets) for (int r = 0; r <= nr && r < capacity_rings; r++) ring_offsets[r] = s.off[(size_t)r];
    if (!xyz || capacity_points <= 0) return VELO_OK;
    HIP_TRY(hipSetDevice(m->device));
    if (m->ins_any) HIP_TRY(hipEventSynchronize(m->ins_ev));
    const int w = std::min(s.n, (int)capacity_points);
    std::vector<float4> h((size_t)w);
    HIP_TRY(hipMemcpy(h.data(), m->arena.at(s.blk), sizeof(float4) * (size_t)w, hipMemcpyDeviceToHost));
    for (int i = 0; i < w; i++) { xyz[3 * i] = h[(size_t)i].x; xyz[3 * i + 1] = h[(size_t)i].y; xyz[3 * i + 2] = h[(size_t)i].z; }
    return VELO_OK;
}

int velo_map_load(velo_map* m, velo_ctx* c, const double ref_inv16[16]) {
    if (!m || !c) return fail(VELO_ERR_INVALID, "null argument");
    return map_load_run(&m, &c, 1, ref_inv16);
}

int velo_map_load_batch(velo_map** maps, velo_ctx** ctxs, int32_t n, const double* ref_inv) {
    return map_load_run(maps, ctxs, n, ref_inv);
}

}  // extern "C"
