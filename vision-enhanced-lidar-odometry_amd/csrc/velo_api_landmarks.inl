// velo_api_landmarks.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: the resident landmark store (velo_landmarks_*): the bookkeeping of main.cpp:614-679 and getLandmarksAtFrame
// (velo.h:1132-1160) on the device; the kernels are in velo_landmark_kernels.h.
//
// Who knows what: the DEVICE holds the state the reference keeps (the observation log with its per-landmark chains, obs_count,
// added, the landmarks, the frame constants) and is what velo_landmarks_get reads.  The HOST keeps only what it needs to size a
// call without asking the device: the id list of every (frame, camera), and per id its observation count and whether a
// triangulation has included it (both follow from the calls alone, so they cannot drift from the device's).
struct LmStore {
    int n_cams = 0;
    // device
    DevBuf<velo_tri_obs> log;
    DevBuf<int> prev, head, count;
    DevBuf<float> pts;
    DevBuf<unsigned char> added;
    DevBuf<TriFrame> frames;
    DevBuf<double> cam_t;
    size_t log_len = 0, log_cap = 0, n_ids = 0, id_cap = 0, frame_cap = 0;
    int log_reallocs = 0;
    // host
    PinBuf<TriFrame> h_frames;                      // pinned mirror of the frame table: a pose travels from its own slot
    std::vector<unsigned char> pose_set, frame_seen;
    int n_missing = 0;                              // frames that hold an observation and no pose
    std::unordered_map<int64_t, std::vector<int32_t>> lists;   // frame * 8 + cam -> ids[cam][frame]
    std::vector<int32_t> h_count;
    std::vector<unsigned char> h_added;
    // staging (a batch call uses the first context's): a call's upload and its read-back, laid out call by call (velo_stage_layout.h)
    StagePair in, out;
    Event in_ev;                                    // in.h may be rewritten once this has passed
    DevBuf<velo_tri_obs> d_obs;                     // the gathered observation lists of a call
    std::shared_ptr<void> ba;                       // the work buffers of velo_landmarks_adjust (BaWork, velo_api_ba.inl), made by its first call
};

namespace {

constexpr int kLmMaxCams = 8;
constexpr int kLmMaxId = 1 << 26;
constexpr size_t kLmDefaultLog = 65536;

inline int64_t lm_key(int frame, int cam) { return (int64_t)frame * kLmMaxCams + cam; }

// a device array that keeps its first `used` elements when it grows; what lies beyond them is filled with the byte `fill`
template <typename T>
int lm_regrow(velo_ctx* c, DevBuf<T>* buf, size_t used, size_t want, int fill) {
    DevBuf<T> nb;
    VELO_TRY(nb.reserve(want));
    if (used > 0) HIP_TRY(hipMemcpyAsync(nb.p, buf->p, sizeof(T) * used, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(nb.p + used, fill, sizeof(T) * (nb.cap - used), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));          // the old buffer is freed by the assignment
    *buf = std::move(nb);
    return VELO_OK;
}

int lm_need_store(velo_ctx* c, const char* who) {
    if (!c->lm) return fail(VELO_ERR_STATE, "%s: velo_landmarks_reset has not run on this context", who);
    return VELO_OK;
}

// the ids some camera observed in `frame`, ascending, once each (the std::set of main.cpp:647-653)
void lm_frame_ids(const LmStore& S, int frame, std::vector<int32_t>* out) {
    out->clear();
    for (int cam = 0; cam < S.n_cams; cam++) {
        auto it = S.lists.find(lm_key(frame, cam));
        if (it != S.lists.end()) out->insert(out->end(), it->second.begin(), it->second.end());
    }
    std::sort(out->begin(), out->end());
    out->erase(std::unique(out->begin(), out->end()), out->end());
}

int lm_triangulate_run(velo_ctx** ctxs, int n_ctx, const int32_t* frames, int32_t* ids_out, float* points_out, velo_tri_result* results_out,
                       int32_t capacity, int32_t* n_out) {
    for (int i = 0; i < n_ctx; i++) {
        VELO_TRY(lm_need_store(ctxs[i], "velo_landmarks_triangulate"));
        if (ctxs[i]->lm->n_missing > 0) return fail(VELO_ERR_STATE, "context %d: %d observed frame(s) have no pose: velo_landmarks_set_pose", i, ctxs[i]->lm->n_missing);
    }
    // the landmarks of the call, context-major; landmark l owns off[l + 1] - off[l] gathered observations
    std::vector<LmItem> items;
    std::vector<int> off(1, 0), first(n_ctx + 1, 0);
    std::vector<char> used(n_ctx, 0);
    std::vector<int32_t> ids;
    for (int i = 0; i < n_ctx; i++) {
        const LmStore& S = *ctxs[i]->lm;
        lm_frame_ids(S, frames[i], &ids);
        for (int32_t id : ids) {
            if (S.h_count[(size_t)id] < 3) continue;             // main.cpp:655-657
            items.push_back(LmItem{id, i});
            off.push_back(off.back() + S.h_count[(size_t)id]);
        }
        first[i + 1] = (int)items.size();
        used[i] = first[i + 1] > first[i];
        n_out[i] = first[i + 1] - first[i];
    }
    const int n = (int)items.size();
    if (n == 0) return VELO_OK;
    velo_ctx* c = ctxs[0];
    LmStore* L = c->lm.get();
    HIP_TRY(hipSetDevice(c->device));
    StageLayout in, out;
    const auto units = in.add<LmUnit>((size_t)n_ctx);
    const auto litems = in.add<LmItem>((size_t)n);
    const auto offs = in.add<int>((size_t)n + 1);
    const auto res = out.add<velo_tri_result>((size_t)n);
    const auto pts = out.add<float>(3 * (size_t)n);
    VELO_TRY(L->in_ev.wait_or_create());
    VELO_TRY(L->in.reserve(in.bytes));
    VELO_TRY(L->out.reserve(out.bytes));
    VELO_TRY(L->d_obs.reserve((size_t)off.back()));
    {
        LmUnit* hu = units.in(L->in.h.p);
        std::memset(hu, 0, litems.off);                          // the units and the padding behind them
        for (int i = 0; i < n_ctx; i++) {
            const velo_ctx* ci = ctxs[i];
            const LmStore& S = *ci->lm;
            LmUnit& U = hu[i];
            U.frames = S.frames.p; U.cam_t = S.cam_t.p; U.log = S.log.p; U.prev = S.prev.p; U.head = S.head.p;
            U.pts = S.pts.p; U.added = S.added.p;
            U.P.lm = lm_params(ci->P);
            U.P.loss_a = ci->P.loss_thresh_3D2D; U.P.loss_w = ci->P.weight_3D2D;    // velo.h:1116-1119
        }
        std::memcpy(litems.in(L->in.h.p), items.data(), litems.size());
        std::memcpy(offs.in(L->in.h.p), off.data(), offs.size());
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, &used));
    HIP_TRY(hipMemcpyAsync(L->in.d.p, L->in.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(L->in_ev, c->stream));
    const LmUnit* d_units = units.in(L->in.d.p);
    const LmItem* d_items = litems.in(L->in.d.p);
    const int* d_off = offs.in(L->in.d.p);
    hipLaunchKernelGGL(lm_gather_kernel, dim3((unsigned)n), dim3(64), 0, c->stream, d_units, d_items, d_off, n, L->d_obs.p);
    hipLaunchKernelGGL(lm_solve_kernel, dim3((unsigned)n), dim3(64), 0, c->stream, d_units, d_items, (const velo_tri_obs*)L->d_obs.p, d_off, n, pts.in(L->out.d.p),
                       res.in(L->out.d.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(L->out.h.p, L->out.d.p, out.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const velo_tri_result* h_res = res.in(L->out.h.p);
    const float* h_pts = pts.in(L->out.h.p);
    for (int i = 0; i < n_ctx; i++) {
        LmStore& S = *ctxs[i]->lm;
        const int b = first[i], m = first[i + 1] - b, w = std::min(m, (int)capacity);
        for (int k = 0; k < m; k++) S.h_added[(size_t)items[(size_t)(b + k)].id] = 1;
        for (int k = 0; k < w && ids_out; k++) ids_out[(size_t)i * capacity + k] = items[(size_t)(b + k)].id;
        if (points_out && w > 0) std::memcpy(points_out + 3 * (size_t)i * capacity, h_pts + 3 * (size_t)b, sizeof(float) * 3 * (size_t)w);
        if (results_out && w > 0) std::memcpy(results_out + (size_t)i * capacity, h_res + b, sizeof(velo_tri_result) * (size_t)w);
    }
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)
int velo_landmarks_reset(velo_ctx* c, int32_t n_cams, const float* cam_trans, int32_t log_capacity) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n_cams < 1 || n_cams > kLmMaxCams) return fail(VELO_ERR_INVALID, "%d cameras; 1..%d", n_cams, kLmMaxCams);
    if (!cam_trans) return fail(VELO_ERR_INVALID, "null cam_trans");
    if (log_capacity < 0) return fail(VELO_ERR_INVALID, "negative log capacity");
    for (int k = 0; k < 3 * n_cams; k++) if (!std::isfinite(cam_trans[k])) return fail(VELO_ERR_INVALID, "cam_trans[%d] is not finite", k);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // nothing of the old store is in flight when it goes
    c->lm.reset();
    std::shared_ptr<LmStore> S = std::make_shared<LmStore>();
    S->n_cams = n_cams;
    double hct[3 * kLmMaxCams];
    for (int k = 0; k < 3 * n_cams; k++) hct[k] = (double)cam_trans[k];
    VELO_TRY(S->cam_t.reserve((size_t)3 * kLmMaxCams));
    HIP_TRY(hipMemcpy(S->cam_t.p, hct, sizeof(double) * 3 * (size_t)n_cams, hipMemcpyHostToDevice));
    const size_t want = log_capacity > 0 ? (size_t)log_capacity : kLmDefaultLog;
    VELO_TRY(S->log.reserve(want));
    VELO_TRY(S->prev.reserve(want));
    S->log_cap = want;                                  // the buffers hold a little more; the log reallocates at what was asked for
    c->lm = S;
    return VELO_OK;
}

int velo_landmarks_set_pose(velo_ctx* c, int32_t frame, const double* pose6) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    if (!pose6) return fail(VELO_ERR_INVALID, "null pose");
    for (int k = 0; k < 6; k++) if (!std::isfinite(pose6[k])) return fail(VELO_ERR_INVALID, "pose[%d] is not finite", k);
    VELO_TRY(lm_need_store(c, "velo_landmarks_set_pose"));
    LmStore& S = *c->lm;
    HIP_TRY(hipSetDevice(c->device));
    if ((size_t)frame >= S.frame_cap) {
        // the table grows geometrically: a new pinned mirror and a new device table, filled from the mirror
        const size_t cap = std::max<size_t>({(size_t)frame + 1, 2 * S.frame_cap, 256});
        PinBuf<TriFrame> nh;
        VELO_TRY(nh.reserve(sizeof(TriFrame) * cap));
        std::memset(nh.p, 0, sizeof(TriFrame) * cap);
        HIP_TRY(hipStreamSynchronize(c->stream));      // copies out of the old mirror have landed
        if (S.h_frames.p) std::memcpy(nh.p, S.h_frames.p, sizeof(TriFrame) * S.frame_cap);
        S.h_frames = std::move(nh);
        DevBuf<TriFrame> nd;
        VELO_TRY(nd.reserve(cap));
        S.frames = std::move(nd);
        HIP_TRY(hipMemcpyAsync(S.frames.p, S.h_frames.p, sizeof(TriFrame) * cap, hipMemcpyHostToDevice, c->stream));
        S.frame_cap = cap;
        S.pose_set.resize(std::max(cap, S.pose_set.size()), 0);
        S.frame_seen.resize(std::max(cap, S.frame_seen.size()), 0);
    }
    tri_frame_from_pose(pose6, &S.h_frames.p[frame]);
    HIP_TRY(hipMemcpyAsync(S.frames.p + frame, S.h_frames.p + frame, sizeof(TriFrame), hipMemcpyHostToDevice, c->stream));
    if (!S.pose_set[(size_t)frame]) { S.pose_set[(size_t)frame] = 1; if (S.frame_seen[(size_t)frame]) S.n_missing--; }
    return VELO_OK;
}

int velo_landmarks_observe(velo_ctx* c, int32_t frame, int32_t cam, const int32_t* ids, const float* keypoints_xy, const int32_t* has_depth,
                           const float* kp_with_depth_xyz, int32_t n_with_depth, int32_t n) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    VELO_TRY(check_cam(cam, kLmMaxCams));
    if (n < 0 || n_with_depth < 0) return fail(VELO_ERR_INVALID, "negative count");
    if (n > 0 && (!ids || !keypoints_xy || !has_depth)) return fail(VELO_ERR_INVALID, "null ids / keypoints / has_depth");
    int32_t max_id = -1;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0) return fail(VELO_ERR_INVALID, "entry %d: negative id %d", i, ids[i]);
        if (ids[i] >= kLmMaxId) return fail(VELO_ERR_INVALID, "entry %d: id %d; below %d", i, ids[i], kLmMaxId);
        if (has_depth[i] < -1 || has_depth[i] >= n_with_depth)
            return fail(VELO_ERR_INVALID, "entry %d: has_depth %d outside the cloud of %d points", i, has_depth[i], n_with_depth);
        if (has_depth[i] >= 0 && !kp_with_depth_xyz) return fail(VELO_ERR_INVALID, "entry %d: has_depth %d and a null cloud", i, has_depth[i]);
        max_id = std::max(max_id, ids[i]);
    }
    if (n > 1) {   // an id twice in one call: found in a sorted copy, so nothing is sized by the value of an id
        std::vector<int32_t> sorted(ids, ids + n);
        std::sort(sorted.begin(), sorted.end());
        for (int i = 1; i < n; i++)
            if (sorted[(size_t)i] == sorted[(size_t)i - 1]) return fail(VELO_ERR_INVALID, "id %d appears twice in one call", sorted[(size_t)i]);
    }
    VELO_TRY(lm_need_store(c, "velo_landmarks_observe"));
    LmStore& S = *c->lm;
    if (cam >= S.n_cams) return fail(VELO_ERR_INVALID, "camera %d; the store has %d", cam, S.n_cams);
    if (S.lists.count(lm_key(frame, cam))) return fail(VELO_ERR_INVALID, "frame %d, camera %d has been observed already", frame, cam);
    HIP_TRY(hipSetDevice(c->device));
    // room first: the id tables (main.cpp:614-621), the log, the staging
    const size_t need_ids = std::max(S.n_ids, (size_t)max_id + 1);
    if (need_ids > S.id_cap) {
        const size_t cap = std::max<size_t>({need_ids, 2 * S.id_cap, 4096});
        VELO_TRY(lm_regrow(c, &S.head, S.n_ids, cap, 0xFF));        // -1: no observation yet
        VELO_TRY(lm_regrow(c, &S.count, S.n_ids, cap, 0));
        VELO_TRY(lm_regrow(c, &S.pts, 3 * S.n_ids, 3 * cap, 0));
        VELO_TRY(lm_regrow(c, &S.added, S.n_ids, cap, 0));
        S.id_cap = std::min(std::min(S.head.cap, S.count.cap), std::min(S.pts.cap / 3, S.added.cap));
    }
    if (S.log_len + (size_t)n > S.log_cap) {
        const size_t cap = std::max(S.log_len + (size_t)n, 2 * S.log_cap);
        VELO_TRY(lm_regrow(c, &S.log, S.log_len, cap, 0));
        VELO_TRY(lm_regrow(c, &S.prev, S.log_len, cap, 0xFF));
        S.log_cap = cap;
        S.log_reallocs++;
    }
    StageLayout in;
    const auto obs = in.add<velo_tri_obs>((size_t)n);
    const auto oids = in.add<int>((size_t)n);
    if (n > 0) {
        VELO_TRY(S.in_ev.wait_or_create());
        VELO_TRY(S.in.reserve(in.bytes));
    }
    // the device first, the host's bookkeeping after the last call that can fail: a failed call leaves the store as it was (what a
    // failed launch may have written lies beyond log_len and in id tables whose counts the host does not trust over its own)
    if (n > 0) {
        velo_tri_obs* ho = obs.in(S.in.h.p);
        int* hi = oids.in(S.in.h.p);
        for (int i = 0; i < n; i++) {
            velo_tri_obs& o = ho[i];
            o.frame = frame; o.cam = cam;
            if (has_depth[i] == -1) { o.kind = VELO_TRI_OBS_2D; o.s[0] = keypoints_xy[2 * i]; o.s[1] = keypoints_xy[2 * i + 1]; o.s[2] = 0.0f; }
            else { const float* p = kp_with_depth_xyz + 3 * (size_t)has_depth[i]; o.kind = VELO_TRI_OBS_3D; o.s[0] = p[0]; o.s[1] = p[1]; o.s[2] = p[2]; }
            hi[i] = ids[i];
        }
        HIP_TRY(hipMemcpyAsync(S.in.d.p, S.in.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(S.in_ev, c->stream));
        hipLaunchKernelGGL(lm_append_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, c->stream, (const velo_tri_obs*)obs.in(S.in.d.p), (const int*)oids.in(S.in.d.p), n,
                           (int)S.log_len, S.log.p, S.prev.p, S.head.p, S.count.p);
        HIP_TRY(hipGetLastError());
    }
    if ((size_t)frame >= S.frame_seen.size()) { S.frame_seen.resize((size_t)frame + 1, 0); S.pose_set.resize((size_t)frame + 1, 0); }
    if (!S.frame_seen[(size_t)frame] && n > 0) { S.frame_seen[(size_t)frame] = 1; if (!S.pose_set[(size_t)frame]) S.n_missing++; }
    S.n_ids = need_ids;
    if (S.h_count.size() < S.n_ids) { S.h_count.resize(S.n_ids, 0); S.h_added.resize(S.n_ids, 0); }
    S.lists[lm_key(frame, cam)].assign(ids, ids + n);
    for (int i = 0; i < n; i++) S.h_count[(size_t)ids[i]]++;
    S.log_len += (size_t)n;
    return VELO_OK;
}

int velo_landmarks_triangulate_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames, int32_t* ids_out, float* points_out,
                                     velo_tri_result* results_out, int32_t capacity, int32_t* n_out) {
    // every argument is checked before any context is touched
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    if (!frames) return fail(VELO_ERR_INVALID, "null frames");
    if (!n_out) return fail(VELO_ERR_INVALID, "null n_out");
    if (capacity < 0) return fail(VELO_ERR_INVALID, "negative capacity");
    for (int i = 0; i < n_ctx; i++) VELO_TRY(check_frame(frames[i], "context", i));
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    return lm_triangulate_run(ctxs, n_ctx, frames, ids_out, points_out, results_out, capacity, n_out);
}

int velo_landmarks_triangulate(velo_ctx* c, int32_t frame, int32_t* ids_out, float* points_out, velo_tri_result* results_out, int32_t capacity,
                               int32_t* n_out) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    return velo_landmarks_triangulate_batch(&c, 1, &frame, ids_out, points_out, results_out, capacity, n_out);
}

int velo_landmarks_at_frame(velo_ctx* c, int32_t frame, const double* pose_inv16, int32_t* ids_out, float* xyz_out, int32_t capacity, int32_t* n_out) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    if (!pose_inv16) return fail(VELO_ERR_INVALID, "null pose_inv");
    if (!n_out) return fail(VELO_ERR_INVALID, "null n_out");
    if (capacity < 0) return fail(VELO_ERR_INVALID, "negative capacity");
    for (int k = 0; k < 16; k++) if (!std::isfinite(pose_inv16[k])) return fail(VELO_ERR_INVALID, "pose_inv[%d] is not finite", k);
    VELO_TRY(lm_need_store(c, "velo_landmarks_at_frame"));
    LmStore& S = *c->lm;
    std::vector<int32_t> all, ids;
    lm_frame_ids(S, frame, &all);
    for (int32_t id : all) if (S.h_added[(size_t)id]) ids.push_back(id);      // velo.h:1143
    *n_out = (int32_t)ids.size();
    const int n = std::min((int)ids.size(), (int)capacity);
    if (n == 0 || (!ids_out && !xyz_out)) return VELO_OK;
    if (ids_out) std::memcpy(ids_out, ids.data(), sizeof(int32_t) * (size_t)n);
    if (!xyz_out) return VELO_OK;
    HIP_TRY(hipSetDevice(c->device));
    StageLayout in, out;
    const auto want = in.add<int>((size_t)n);
    const auto xyz = out.add<float>(3 * (size_t)n);
    VELO_TRY(S.in_ev.wait_or_create());
    VELO_TRY(S.in.reserve(in.bytes));
    VELO_TRY(S.out.reserve(out.bytes));
    std::memcpy(want.in(S.in.h.p), ids.data(), want.size());
    LmPose M;
    std::memcpy(M.m, pose_inv16, sizeof(M.m));
    HIP_TRY(hipMemcpyAsync(S.in.d.p, S.in.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(S.in_ev, c->stream));
    hipLaunchKernelGGL(lm_at_frame_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, c->stream, (const int*)want.in(S.in.d.p), n, (const float*)S.pts.p, M, xyz.in(S.out.d.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(S.out.h.p, S.out.d.p, out.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(xyz_out, xyz.in(S.out.h.p), xyz.size());
    return VELO_OK;
}

int velo_landmarks_get(velo_ctx* c, const int32_t* ids, int32_t n, float* xyz, uint8_t* added, int32_t* obs_count) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n < 0) return fail(VELO_ERR_INVALID, "negative count");
    if (n > 0 && !ids) return fail(VELO_ERR_INVALID, "null ids");
    for (int i = 0; i < n; i++) if (ids[i] < 0) return fail(VELO_ERR_INVALID, "entry %d: negative id %d", i, ids[i]);
    VELO_TRY(lm_need_store(c, "velo_landmarks_get"));
    if (n == 0) return VELO_OK;
    LmStore& S = *c->lm;
    HIP_TRY(hipSetDevice(c->device));
    StageLayout in, out;
    const auto want = in.add<int>((size_t)n);
    const auto oxyz = out.add<float>(3 * (size_t)n);             // the three arrays packed
    const auto ocnt = out.add<int>((size_t)n, 4);
    const auto oadd = out.add<unsigned char>((size_t)n, 1);
    VELO_TRY(S.in_ev.wait_or_create());
    VELO_TRY(S.in.reserve(in.bytes));
    VELO_TRY(S.out.reserve(out.bytes));
    std::memcpy(want.in(S.in.h.p), ids, want.size());
    HIP_TRY(hipMemcpyAsync(S.in.d.p, S.in.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(S.in_ev, c->stream));
    hipLaunchKernelGGL(lm_get_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, c->stream, (const int*)want.in(S.in.d.p), n, (int)S.n_ids, (const float*)S.pts.p,
                       (const unsigned char*)S.added.p, (const int*)S.count.p, oxyz.in(S.out.d.p), ocnt.in(S.out.d.p), oadd.in(S.out.d.p));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(S.out.h.p, S.out.d.p, out.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (xyz) std::memcpy(xyz, oxyz.in(S.out.h.p), oxyz.size());
    if (obs_count) std::memcpy(obs_count, ocnt.in(S.out.h.p), ocnt.size());
    if (added) std::memcpy(added, oadd.in(S.out.h.p), oadd.size());
    return VELO_OK;
}

int velo_landmarks_frame_count(velo_ctx* c, int32_t frame, int32_t* n_seen, int32_t* n_to_triangulate) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    VELO_TRY(lm_need_store(c, "velo_landmarks_frame_count"));
    const LmStore& S = *c->lm;
    std::vector<int32_t> ids;
    lm_frame_ids(S, frame, &ids);
    int m = 0;
    for (int32_t id : ids) m += S.h_count[(size_t)id] >= 3 ? 1 : 0;
    if (n_seen) *n_seen = (int32_t)ids.size();
    if (n_to_triangulate) *n_to_triangulate = m;
    return VELO_OK;
}

int velo_landmarks_info(velo_ctx* c, int32_t* info) {
    if (!c || !info) return fail(VELO_ERR_INVALID, "null argument");
    VELO_TRY(lm_need_store(c, "velo_landmarks_info"));
    const LmStore& S = *c->lm;
    info[0] = (int32_t)S.n_ids; info[1] = (int32_t)S.log_len; info[2] = (int32_t)S.log_cap; info[3] = S.log_reallocs;
    info[4] = (int32_t)S.frame_cap; info[5] = S.n_cams; info[6] = (int32_t)S.lists.size(); info[7] = 0;
    return VELO_OK;
}

}  // extern "C"
