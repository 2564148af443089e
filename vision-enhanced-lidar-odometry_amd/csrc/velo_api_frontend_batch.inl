// velo_api_frontend_batch.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: the visual front end of SEVERAL contexts in one call each -- velo_set_images_batch, velo_track_features_batch,
// velo_detect_features_batch; the batch kernels are in velo_track_kernels.h / velo_detect_kernels.h.
//
// Who owns what: the FIRST context of a call (ctxs[0]) lends its stream, its pinned staging and its scratch buffers (lk_raw / lk_in / lk_out,
// gf_*); every context keeps its own image slots, and the kernels write / read them through per-unit tables.  Mixed image sizes are
// served by the SAME launches: a table entry carries its unit's size, grids are sized for the largest unit.
// Hand-over between the streams: the lending stream first waits for an event recorded on every other named context's stream; the
// synchronous entries (track, detect) end in a synchronisation of the lending stream, after which nothing of the call is in flight;
// the asynchronous one (set_images) records an event on the lending stream that every other context's stream then waits for.
namespace {

constexpr int kFbMaxCtx = 256;             // contexts per call
constexpr int kFbDetectUnits = 64;         // cameras per detection launch set (a call with more runs in chunks)
constexpr int kFbHdrStride = 32;           // ints between the headers of two units: a 128-byte line each, so that the per-workgroup atomics
                                           // of different units (candidate counts, maxima) do not queue on one line

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

int fb_check_job_ctx(const int32_t* job_ctx, int n_jobs, int n_ctx) {
    if (!job_ctx) return fail(VELO_ERR_INVALID, "null job_ctx");
    for (int j = 0; j < n_jobs; j++)
        if (job_ctx[j] < 0 || job_ctx[j] >= n_ctx) return fail(VELO_ERR_INVALID, "job %d: context index %d; 0..%d", j, job_ctx[j], n_ctx - 1);
    return VELO_OK;
}

// the lending stream runs after everything already enqueued on the stream of every other context in `used` (null: all)
int fb_gather(velo_ctx** ctxs, int n_ctx, const std::vector<char>* used) {
    velo_ctx* c0 = ctxs[0];
    for (int i = 1; i < n_ctx; i++) {
        if (used && !(*used)[i]) continue;
        velo_ctx* c = ctxs[i];
        if (c->stream == c0->stream) continue;
        if (!c->fb_here_ev) HIP_TRY(hipEventCreateWithFlags(&c->fb_here_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->fb_here_ev, c->stream));
        HIP_TRY(hipStreamWaitEvent(c0->stream, c->fb_here_ev, 0));
    }
    return VELO_OK;
}

// whatever is enqueued later on any other context's stream runs after what the lending stream holds now
int fb_release(velo_ctx** ctxs, int n_ctx) {
    velo_ctx* c0 = ctxs[0];
    if (n_ctx < 2) return VELO_OK;
    if (!c0->fb_done_ev) HIP_TRY(hipEventCreateWithFlags(&c0->fb_done_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c0->fb_done_ev, c0->stream));
    for (int i = 1; i < n_ctx; i++)
        if (ctxs[i]->stream != c0->stream) HIP_TRY(hipStreamWaitEvent(ctxs[i]->stream, c0->fb_done_ev, 0));
    return VELO_OK;
}

// index of the level table of a w x h image in `pyrs` (appended when new)
int fb_pyr_index(std::vector<LkPyr>* pyrs, std::vector<long long>* cam_pix, int w, int h) {
    for (size_t k = 0; k < pyrs->size(); k++) if ((*pyrs)[k].lv[0].w == w && (*pyrs)[k].lv[0].h == h) return (int)k;
    LkPyr P;
    long long cp = 0;
    lk_plan(&P, w, h, &cp);
    pyrs->push_back(P);
    cam_pix->push_back(cp);
    return (int)pyrs->size() - 1;
}

inline size_t fb_align64(size_t n) { return (n + 63) & ~(size_t)63; }

// one launch set of detection: the units [u0, u0 + nu) of the call and the jobs `sel` that name them (call order)
struct FbDetectUnit { int ctx, cam; };
int fb_detect_run(velo_ctx** ctxs, int n_ctx, const std::vector<FbDetectUnit>& units, int u0, int nu, const std::vector<int>& unit_of_job, const std::vector<int>& sel,
                  const velo_detect_job* jobs, const velo_gftt_params* p, int32_t capacity, float* xy, float* response, uint8_t* fresh, int32_t* counts) {
    velo_ctx* c = ctxs[0];
    const int nj = (int)sel.size();
    // every unit's share of the scratch buffers: sizes differ, so offsets are summed, not multiplied
    std::vector<size_t> plane(nu), splane(nu), kcap(nu), o_plane(nu), o_state(nu), o_keys(nu);
    std::vector<int> sstride(nu);
    size_t t_plane = 0, t_state = 0, t_keys = 0, max_plane = 0;
    int max_w = 0, max_h = 0;
    for (int u = 0; u < nu; u++) {
        const LkSlot& S = *lk_slot(ctxs[units[u0 + u].ctx], false);
        plane[u] = (size_t)S.w * S.h;
        sstride[u] = (S.w + 2 * kGfStatePad + 3) & ~3;
        splane[u] = (size_t)sstride[u] * (S.h + 2 * kGfStatePad);
        kcap[u] = 1;
        while (kcap[u] < plane[u]) kcap[u] <<= 1;
        o_plane[u] = t_plane; o_state[u] = t_state; o_keys[u] = t_keys;
        t_plane += plane[u]; t_state += splane[u]; t_keys += kcap[u];
        max_plane = std::max(max_plane, plane[u]);
        max_w = std::max(max_w, S.w); max_h = std::max(max_h, S.h);
    }
    const int cap_d = (int)std::min<size_t>((size_t)capacity, max_plane);     // a camera has at most one corner per pixel
    VELO_TRY(c->gf_eig.reserve(t_plane));
    VELO_TRY(c->gf_state.reserve(t_state));
    VELO_TRY(c->gf_cand.reserve(2 * t_plane));
    VELO_TRY(c->gf_keys.reserve(t_keys));
    VELO_TRY(c->gf_hdr.reserve(std::max((size_t)kFbHdrStride * nu, (size_t)kGfHdr * kGfMaxUnits)));
    GfParams K;
    std::memset(&K, 0, sizeof(K));
    const float s = (float)(1.0 / (255.0 * 4.0 * 3.0));       // cornerMinEigenVal: 1 / (255 * 2^(ksize - 1) * blockSize)
    K.scale2 = s * s;
    K.radius = (int)std::ceil(p->min_distance) - 1;
    K.max_corners = p->max_corners;
    K.capacity = cap_d;
    K.quality = p->quality_level;
    K.md2 = p->min_distance * p->min_distance;
    K.md2f = (float)(p->min_distance * p->min_distance);
    int64_t total = 0;
    for (int k = 0; k < nj; k++) total += jobs[sel[k]].n_existing;
    const size_t unit_bytes = fb_align64(sizeof(GfUnit) * (size_t)nu);
    const size_t job_bytes = fb_align64(sizeof(GfJob) * (size_t)nj);
    const size_t in_bytes = unit_bytes + job_bytes + sizeof(float2) * (size_t)total;
    const size_t cnt_bytes = fb_align64(sizeof(int) * 3 * (size_t)nj);
    const size_t n_slots = (size_t)nj * cap_d;
    const size_t out_bytes = cnt_bytes + n_slots * (sizeof(float2) + sizeof(float) + 1);
    VELO_TRY(match_pinned((void**)&c->h_gf_in, &c->h_gf_in_cap, in_bytes));
    VELO_TRY(match_pinned((void**)&c->h_gf_out, &c->h_gf_out_cap, out_bytes));
    VELO_TRY(c->gf_in.reserve(in_bytes));
    VELO_TRY(c->gf_out.reserve(out_bytes));
    {
        GfUnit* hu = (GfUnit*)c->h_gf_in;
        for (int u = 0; u < nu; u++) {
            const LkSlot& S = *lk_slot(ctxs[units[u0 + u].ctx], false);
            GfUnit& U = hu[u];
            U.plane = S.pix.p + (size_t)units[u0 + u].cam * S.cam_pix + S.pyr.lv[0].off;
            U.eig = c->gf_eig.p + o_plane[u];
            U.state = c->gf_state.p + o_state[u];
            U.cand = c->gf_cand.p + o_plane[u];
            U.und = c->gf_cand.p + t_plane + o_plane[u];
            U.keys = c->gf_keys.p + o_keys[u];
            U.hdr = c->gf_hdr.p + (size_t)u * kFbHdrStride;
            U.w = S.w; U.h = S.h; U.stride = S.pyr.lv[0].stride; U.sstride = sstride[u];
        }
        GfJob* hj = (GfJob*)(c->h_gf_in + unit_bytes);
        float* hp = (float*)(c->h_gf_in + unit_bytes + job_bytes);
        int first = 0;
        for (int k = 0; k < nj; k++) {
            const velo_detect_job& J = jobs[sel[k]];
            hj[k].unit = unit_of_job[sel[k]] - u0; hj[k].first = first; hj[k].n = J.n_existing; hj[k].pad_ = 0;
            if (J.n_existing > 0) std::memcpy(hp + 2 * (size_t)first, J.existing_xy, sizeof(float) * 2 * (size_t)J.n_existing);
            first += J.n_existing;
        }
    }
    std::vector<char> used(n_ctx, 0);
    for (int u = 0; u < nu; u++) used[units[u0 + u].ctx] = 1;
    VELO_TRY(fb_gather(ctxs, n_ctx, &used));
    HIP_TRY(hipMemcpyAsync(c->gf_in.p, c->h_gf_in, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->gf_hdr.p, 0, sizeof(int) * kFbHdrStride * (size_t)nu, c->stream));
    HIP_TRY(hipMemsetAsync(c->gf_state.p, 0, t_state, c->stream));                          // the zero border of the state maps
    HIP_TRY(hipMemsetAsync(c->gf_out.p, 0, cnt_bytes, c->stream));
    const GfUnit* d_units = (const GfUnit*)c->gf_in.p;
    hipLaunchKernelGGL(gf_response_batch_kernel, dim3((unsigned)cdiv(max_w, kGfTile), (unsigned)cdiv(max_h, kGfTile), (unsigned)nu), dim3(kGfTile * kGfTile), 0,
                       c->stream, d_units, K);
    hipLaunchKernelGGL(gf_candidates_batch_kernel, dim3((unsigned)cdiv(max_w, 64), (unsigned)cdiv(max_h, 4), (unsigned)nu), dim3(256), 0, c->stream, d_units, K);
    for (int r = 0; r < kGfRoundLaunches; r++)
        hipLaunchKernelGGL(gf_round_batch_kernel, dim3(kGfRoundBlocks, (unsigned)nu), dim3(256), 0, c->stream, d_units, K);
    hipLaunchKernelGGL(gf_finish_batch_kernel, dim3((unsigned)nu), dim3(kGfFinishThreads), 0, c->stream, d_units, K);
    int* d_counts = (int*)c->gf_out.p;
    float2* d_xy = (float2*)(c->gf_out.p + cnt_bytes);
    float* d_resp = (float*)(c->gf_out.p + cnt_bytes + n_slots * sizeof(float2));
    unsigned char* d_fresh = c->gf_out.p + cnt_bytes + n_slots * (sizeof(float2) + sizeof(float));
    hipLaunchKernelGGL(gf_output_batch_kernel, dim3(kGfOutBlocks, (unsigned)nj), dim3(256), 0, c->stream, d_units, K, (const GfJob*)(c->gf_in.p + unit_bytes),
                       (const float2*)(c->gf_in.p + unit_bytes + job_bytes), d_counts, d_xy, d_resp, d_fresh);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_gf_out, c->gf_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->gf_units = 0;                                         // the headers are other contexts' and laid out differently: nothing for velo_diag_detect_counters
    const int* h_counts = (const int*)c->h_gf_out;
    const unsigned char* h_xy = c->h_gf_out + cnt_bytes;
    const unsigned char* h_resp = h_xy + n_slots * sizeof(float2);
    const unsigned char* h_fresh = h_resp + n_slots * sizeof(float);
    for (int k = 0; k < nj; k++) {
        const size_t j = (size_t)sel[k];
        std::memcpy(counts + 3 * j, h_counts + 3 * k, sizeof(int) * 3);
        const size_t m = (size_t)std::min(h_counts[3 * k], cap_d);            // what lies past it in the caller's arrays stays as it was
        if (m == 0) continue;
        std::memcpy(xy + 2 * j * capacity, h_xy + sizeof(float2) * (size_t)k * cap_d, sizeof(float2) * m);
        std::memcpy(response + j * capacity, h_resp + sizeof(float) * (size_t)k * cap_d, sizeof(float) * m);
        std::memcpy(fresh + j * capacity, h_fresh + (size_t)k * cap_d, m);
    }
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)
int velo_set_images_batch(velo_ctx** ctxs, int32_t n_ctx, const uint8_t* const* imgs, int32_t n_cams, const int32_t* sizes) {
    // every argument is checked before any context is touched
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    if (n_cams < 1 || n_cams > kLkMaxCams) return fail(VELO_ERR_INVALID, "%d cameras; 1..%d", n_cams, kLkMaxCams);
    if (!imgs) return fail(VELO_ERR_INVALID, "null image list");
    if (!sizes) return fail(VELO_ERR_INVALID, "null sizes");
    for (int i = 0; i < n_ctx; i++) {
        for (int k = 0; k < n_cams; k++) if (!imgs[(size_t)i * n_cams + k]) return fail(VELO_ERR_INVALID, "context %d: image %d is null", i, k);
        const int w = sizes[3 * i], h = sizes[3 * i + 1], st = sizes[3 * i + 2];
        if (w < 1 || h < 1 || w > 16384 || h > 16384) return fail(VELO_ERR_INVALID, "context %d: image size %d x %d; 1..16384 each", i, w, h);
        if (st < w) return fail(VELO_ERR_INVALID, "context %d: row stride %d < width %d", i, st, w);
    }
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    if (n_ctx == 1) return velo_set_images(ctxs[0], imgs, n_cams, sizes[0], sizes[1], sizes[2]);
    velo_ctx* c = ctxs[0];
    HIP_TRY(hipSetDevice(c->device));
    // the pinned staging buffer may still be read by the previous call's upload
    if (c->lk_upload_ev) HIP_TRY(hipEventSynchronize(c->lk_upload_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->lk_upload_ev, hipEventDisableTiming));
    std::vector<LkPyr> pyrs;
    std::vector<long long> cam_pix;
    std::vector<int> pyr_of(n_ctx);
    size_t raw_bytes = 0;
    for (int i = 0; i < n_ctx; i++) {
        pyr_of[i] = fb_pyr_index(&pyrs, &cam_pix, sizes[3 * i], sizes[3 * i + 1]);
        raw_bytes += (size_t)n_cams * sizes[3 * i] * sizes[3 * i + 1];
    }
    const int n_units = n_ctx * n_cams;
    const size_t unit_bytes = fb_align64(sizeof(LkBuildUnit) * (size_t)n_units);
    const size_t pyr_bytes = fb_align64(sizeof(LkPyr) * pyrs.size());
    const size_t in_bytes = unit_bytes + pyr_bytes + raw_bytes;
    VELO_TRY(match_pinned((void**)&c->h_lk_raw, &c->h_lk_raw_cap, in_bytes));
    VELO_TRY(c->lk_raw.reserve(in_bytes));
    // the slot every context is about to fill: its previous one (current -> previous is a rotation, no copy)
    // every allocation first: a failure leaves every context's images as they were, except a slot whose buffer had to be replaced
    for (int i = 0; i < n_ctx; i++) {
        LkSlot& S = ctxs[i]->lk_slot[ctxs[i]->lk_cur ^ 1];
        const size_t need = (size_t)cam_pix[pyr_of[i]] * n_cams;
        if (need > S.pix.cap || need > S.der.cap) S.valid = false;   // growing frees the old buffer: that slot's images are gone either way
        VELO_TRY(S.pix.reserve(need));
        VELO_TRY(S.der.reserve(need));
    }
    for (int i = 0; i < n_ctx; i++) ctxs[i]->lk_slot[ctxs[i]->lk_cur ^ 1].valid = false;
    {
        LkBuildUnit* hu = (LkBuildUnit*)c->h_lk_raw;
        std::memcpy(c->h_lk_raw + unit_bytes, pyrs.data(), sizeof(LkPyr) * pyrs.size());
        size_t off = unit_bytes + pyr_bytes;
        for (int i = 0; i < n_ctx; i++) {
            const int w = sizes[3 * i], h = sizes[3 * i + 1], st = sizes[3 * i + 2];
            LkSlot& S = ctxs[i]->lk_slot[ctxs[i]->lk_cur ^ 1];
            for (int k = 0; k < n_cams; k++) {
                LkBuildUnit& U = hu[i * n_cams + k];
                U.raw = c->lk_raw.p + off;
                U.pix = S.pix.p + (size_t)k * cam_pix[pyr_of[i]];
                U.der = S.der.p + (size_t)k * cam_pix[pyr_of[i]];
                U.pyr = pyr_of[i]; U.pad_ = 0;
                const uint8_t* src = imgs[(size_t)i * n_cams + k];
                for (int y = 0; y < h; y++) std::memcpy(c->h_lk_raw + off + (size_t)y * w, src + (size_t)y * st, (size_t)w);
                off += (size_t)w * h;
            }
        }
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, nullptr));
    HIP_TRY(hipMemcpyAsync(c->lk_raw.p, c->h_lk_raw, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->lk_upload_ev, c->stream));
    int max_levels = 0;
    for (const LkPyr& P : pyrs) max_levels = std::max(max_levels, P.n_levels);
    for (int lev = 0; lev < max_levels; lev++) {
        int mw = 0, mh = 0;                                   // the largest unit that has this level
        for (const LkPyr& P : pyrs) if (lev < P.n_levels) { mw = std::max(mw, P.lv[lev].w); mh = std::max(mh, P.lv[lev].h); }
        const dim3 grid((unsigned)cdiv(mw + 2 * kLkPad, kLkTile), (unsigned)cdiv(mh + 2 * kLkPad, kLkTile), (unsigned)n_units);
        hipLaunchKernelGGL(lk_build_batch_kernel, grid, dim3(kLkTile * kLkTile), 0, c->stream, (const LkBuildUnit*)c->lk_raw.p,
                           (const LkPyr*)(c->lk_raw.p + unit_bytes), lev);
    }
    HIP_TRY(hipGetLastError());
    VELO_TRY(fb_release(ctxs, n_ctx));
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* ci = ctxs[i];
        ci->lk_cur ^= 1;
        LkSlot& S = ci->lk_slot[ci->lk_cur];
        S.pyr = pyrs[pyr_of[i]]; S.cam_pix = cam_pix[pyr_of[i]]; S.n_cams = n_cams; S.w = sizes[3 * i]; S.h = sizes[3 * i + 1]; S.valid = true;
    }
    return VELO_OK;
}

int velo_track_features_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* job_ctx, const velo_track_job* jobs, int32_t n_jobs,
                              const velo_lk_params* p, float* next_xy, uint8_t* status, uint8_t* kept) {
    // every argument is checked before any context is touched
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    VELO_TRY(lk_check_params(n_jobs, p));
    if (n_jobs == 0) return VELO_OK;
    int64_t total = 0;
    VELO_TRY(lk_check_jobs(jobs, n_jobs, next_xy, status, kept, &total));
    VELO_TRY(fb_check_job_ctx(job_ctx, n_jobs, n_ctx));
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    if (n_ctx == 1) return velo_track_features(ctxs[0], jobs, n_jobs, p, next_xy, status, kept);
    std::vector<char> used(n_ctx, 0);
    for (int j = 0; j < n_jobs; j++) {
        const int i = job_ctx[j];
        const LkSlot& Sp = *lk_slot(ctxs[i], true);
        const LkSlot& Sc = *lk_slot(ctxs[i], false);
        if (!used[i]) {
            if (!Sp.valid || !Sc.valid) return fail(VELO_ERR_STATE, "context %d: tracking needs a previous and a current frame: velo_set_images twice", i);
            if (Sp.w != Sc.w || Sp.h != Sc.h || Sp.cam_pix != Sc.cam_pix)
                return fail(VELO_ERR_INVALID, "context %d: previous images are %d x %d, current %d x %d", i, Sp.w, Sp.h, Sc.w, Sc.h);
            used[i] = 1;
        }
        if (jobs[j].prev_cam < 0 || jobs[j].prev_cam >= Sp.n_cams || jobs[j].cam < 0 || jobs[j].cam >= Sc.n_cams)
            return fail(VELO_ERR_INVALID, "job %d: cameras (%d -> %d) outside the %d / %d that context %d uploaded", j, jobs[j].prev_cam, jobs[j].cam, Sp.n_cams,
                        Sc.n_cams, i);
    }
    if (total == 0) return VELO_OK;
    const int n = (int)total;
    velo_ctx* c = ctxs[0];
    HIP_TRY(hipSetDevice(c->device));
    std::vector<LkPyr> pyrs;
    std::vector<long long> cam_pix;
    std::vector<int> pyr_of(n_ctx, -1);
    for (int i = 0; i < n_ctx; i++) if (used[i]) pyr_of[i] = fb_pyr_index(&pyrs, &cam_pix, lk_slot(ctxs[i], false)->w, lk_slot(ctxs[i], false)->h);
    const size_t job_bytes = fb_align64(sizeof(LkBatchJob) * (size_t)n_jobs);
    const size_t pyr_bytes = fb_align64(sizeof(LkPyr) * pyrs.size());
    const size_t in_bytes = job_bytes + pyr_bytes + sizeof(float2) * (size_t)n;
    const size_t out_bytes = sizeof(float2) * (size_t)n + 2 * (size_t)n;
    VELO_TRY(match_pinned((void**)&c->h_lk_in, &c->h_lk_in_cap, in_bytes));
    VELO_TRY(match_pinned((void**)&c->h_lk_out, &c->h_lk_out_cap, out_bytes));
    VELO_TRY(c->lk_in.reserve(in_bytes));
    VELO_TRY(c->lk_out.reserve(out_bytes));
    {
        LkBatchJob* hj = (LkBatchJob*)c->h_lk_in;
        std::memcpy(c->h_lk_in + job_bytes, pyrs.data(), sizeof(LkPyr) * pyrs.size());
        float* hp = (float*)(c->h_lk_in + job_bytes + pyr_bytes);
        int first = 0;
        for (int j = 0; j < n_jobs; j++) {
            const int i = job_ctx[j];
            const LkSlot& Sp = *lk_slot(ctxs[i], true);
            const LkSlot& Sc = *lk_slot(ctxs[i], false);
            hj[j].first = first; hj[j].n = jobs[j].n;
            hj[j].pyr = pyr_of[i];
            hj[j].top = std::min(lk_level_count(Sc.w, Sc.h, p->window, p->max_level), Sc.pyr.n_levels - 1);
            hj[j].prev_pix = Sp.pix.p + (size_t)jobs[j].prev_cam * Sp.cam_pix;
            hj[j].prev_der = Sp.der.p + (size_t)jobs[j].prev_cam * Sp.cam_pix;
            hj[j].cur_pix = Sc.pix.p + (size_t)jobs[j].cam * Sc.cam_pix;
            if (jobs[j].n > 0) std::memcpy(hp + 2 * (size_t)first, jobs[j].prev_xy, sizeof(float) * 2 * (size_t)jobs[j].n);
            first += jobs[j].n;
        }
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, &used));
    HIP_TRY(hipMemcpyAsync(c->lk_in.p, c->h_lk_in, in_bytes, hipMemcpyHostToDevice, c->stream));
    LkParams K;
    std::memset(&K, 0, sizeof(K));
    K.win = p->window; K.max_count = p->max_count;
    K.min_eig = (float)p->min_eig_threshold;
    K.eps2 = p->epsilon * p->epsilon;
    K.flow_outlier = p->flow_outlier;
    const LkBatchJob* djobs = (const LkBatchJob*)c->lk_in.p;
    const LkPyr* dpyrs = (const LkPyr*)(c->lk_in.p + job_bytes);
    const float2* dpts = (const float2*)(c->lk_in.p + job_bytes + pyr_bytes);
    float2* oxy = (float2*)c->lk_out.p;
    unsigned char* ost = c->lk_out.p + sizeof(float2) * (size_t)n;
    unsigned char* okp = ost + n;
    const dim3 grid((unsigned)cdiv(n, kLkThreads / 64));
    const int npl = cdiv(p->window * p->window, 64);
    if (npl <= 4)
        hipLaunchKernelGGL(lk_track_batch_kernel_4, grid, dim3(kLkThreads), 0, c->stream, djobs, n_jobs, dpyrs, dpts, n, K, oxy, ost, okp);
    else if (npl <= 8)
        hipLaunchKernelGGL(lk_track_batch_kernel_8, grid, dim3(kLkThreads), 0, c->stream, djobs, n_jobs, dpyrs, dpts, n, K, oxy, ost, okp);
    else
        hipLaunchKernelGGL(lk_track_batch_kernel_16, grid, dim3(kLkThreads), 0, c->stream, djobs, n_jobs, dpyrs, dpts, n, K, oxy, ost, okp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_lk_out, c->lk_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(next_xy, c->h_lk_out, sizeof(float2) * (size_t)n);
    std::memcpy(status, c->h_lk_out + sizeof(float2) * (size_t)n, (size_t)n);
    std::memcpy(kept, c->h_lk_out + sizeof(float2) * (size_t)n + n, (size_t)n);
    return VELO_OK;
}

int velo_detect_features_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* job_ctx, const velo_detect_job* jobs, int32_t n_jobs,
                               const velo_gftt_params* p, int32_t capacity, float* xy, float* response, uint8_t* fresh, int32_t* counts) {
    // every argument is checked before any context is touched
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    VELO_TRY(gf_check_params(n_jobs, p, capacity));
    if (n_jobs == 0) return VELO_OK;
    int64_t total = 0;
    VELO_TRY(gf_check_jobs(jobs, n_jobs, capacity, xy, response, fresh, counts, &total));
    VELO_TRY(fb_check_job_ctx(job_ctx, n_jobs, n_ctx));
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    if (n_ctx == 1) return velo_detect_features(ctxs[0], jobs, n_jobs, p, capacity, xy, response, fresh, counts);
    // the units: the distinct (context, camera) pairs, in the order the jobs name them
    std::vector<FbDetectUnit> units;
    std::vector<int> unit_of_job(n_jobs), unit_at((size_t)n_ctx * kLkMaxCams, -1);
    for (int j = 0; j < n_jobs; j++) {
        const int i = job_ctx[j];
        const LkSlot& S = *lk_slot(ctxs[i], false);
        if (!S.valid) return fail(VELO_ERR_STATE, "context %d: no current images: velo_set_images first", i);
        if (jobs[j].cam >= S.n_cams) return fail(VELO_ERR_INVALID, "job %d: camera %d outside the %d that context %d uploaded", j, jobs[j].cam, S.n_cams, i);
        int& u = unit_at[(size_t)i * kLkMaxCams + jobs[j].cam];
        if (u < 0) { u = (int)units.size(); units.push_back(FbDetectUnit{i, jobs[j].cam}); }
        unit_of_job[j] = u;
    }
    HIP_TRY(hipSetDevice(ctxs[0]->device));
    std::vector<int> sel;
    for (int u0 = 0; u0 < (int)units.size(); u0 += kFbDetectUnits) {
        const int nu = std::min(kFbDetectUnits, (int)units.size() - u0);
        sel.clear();
        for (int j = 0; j < n_jobs; j++) if (unit_of_job[j] >= u0 && unit_of_job[j] < u0 + nu) sel.push_back(j);
        VELO_TRY(fb_detect_run(ctxs, n_ctx, units, u0, nu, unit_of_job, sel, jobs, p, capacity, xy, response, fresh, counts));
    }
    return VELO_OK;
}

}  // extern "C"
