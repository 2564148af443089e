// velo_api_frames.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: resident keypoint frames (velo_frames_*) and the assembly of frameToFrame's visual matches from them
// (velo_build_matches[_batch], velo_get_visual): matchUsingId (velo.h:562-590), the landmark substitution and the gather of
// velo.h:627-654 on the device; the kernels are in velo_frame_kernels.h.  Also the frames' descriptor rows (velo_frames_put_descriptors),
// the visual set of a loop-closure edge joined by them (velo_build_matches_desc[_batch]: matchFeatures, velo.h:499-560, on the match
// kernels of velo_match_kernels.h) and the screening of a frame against many candidates (velo_match_frames).  Also the prune of a frame
// to a registration's good matches (velo_frames_prune / _keep) and the put of a frame whose keypoint depth the device computes
// (velo_frames_put_frame[_batch]: velo.h:329-497 on the device functions of velo_depth_kernels.h, in front of this store and the landmark store).
//
// Who knows what: the DEVICE holds the arrays of every (frame, camera) in one arena of 4-byte words and one slot table per camera;
// the HOST keeps the directory (frame, cam) -> block, n, n_with_depth, the largest id of the block (which sizes the slot table
// without asking the device) and the list of free blocks.  The free list is first-fit and neither splits nor merges blocks: it is
// made for the reference's use, a sliding window of frames of similar size (3,000 keypoints per camera, kitti.h) in which a dropped
// frame's blocks are taken by the next frame's entries of about the same size; a caller that mixes very different sizes pays with
// arena growth (velo_frames_info shows it), never with wrong results.
// The descriptor rows of a (frame, camera) live in a second arena of 64-byte rows with a directory and a free list of its own, under
// the same rules; the keypoint arena does not know of it.

// Both arenas are an FrArena: the device buffer with its bookkeeping (velo_block_list.h), in words (the caller rounds to 16) or rows of four uint4.
template <typename T, size_t Per>                    // Per elements of T to a unit
struct FrArena {
    DevBuf<T> buf;
    BlockList list;
    T* at(const Block& b) const { return buf.p + Per * b.off; }
    // where an entry of `need` units goes (old: the block it holds now, or null); the arena has grown if the plan asked for it, and
    // nothing else of the bookkeeping has changed: list.commit(plan, old) follows the last call that can fail
    int place(velo_ctx* c, const Block* old, size_t need, BlockList::Plan* plan) { return place(c, &list, old, need, plan); }
    // the same on a copy of the bookkeeping: a call that places several entries and fails on a later one hands no list back
    int place(velo_ctx* c, BlockList* l, const Block* old, size_t need, BlockList::Plan* plan) {
        *plan = l->plan(old, need);
        if (plan->grow_to > 0) {
            VELO_TRY(lm_regrow(c, &buf, Per * l->used, Per * plan->grow_to, 0));
            l->grew(*plan);
        }
        return VELO_OK;
    }
};

struct FrStore {
    int n_cams = 0;
    float cam_t[3 * 8] = {};
    // device
    FrArena<int, 1> kp;                             // the keypoint arrays; every block starts on a 64-byte line
    DevBuf<int> slots;                              // n_cams tables of slot_ids entries, all -1 between calls
    size_t slot_ids = 0;
    bool slots_dirty = false;                       // a call failed between the fill and the clear launch: refill before the next one
    FrArena<uint4, 4> rows;                         // the descriptor rows, 64 bytes each
    DevBuf<unsigned> d_keys;                        // nearest-row keys and min_dist of a descriptor-matched call
    // host: the directories, frame * 8 + cam -> block
    struct Entry { Block blk; int n = 0, n_wd = 0, max_id = -1; uint64_t gen = 0; };   // gen: a stamp no two versions of any entry share
    std::unordered_map<int64_t, Entry> dir;
    struct RowEntry { Block blk; int n = 0; };
    std::unordered_map<int64_t, RowEntry> rdir;
    PinStage put_stage, rows_stage;                 // staging of velo_frames_put and of velo_frames_put_descriptors
    // staging of the launch sets (a batch call uses the first context's), laid out call by call (velo_stage_layout.h); every call ends in a synchronisation, so nothing guards it
    StagePair in, out;
    DevBuf<unsigned char> d_prune;                  // scratch of a prune call: the keep maps | the gathered blocks | the gathered rows
    // scratch of a frame put with its depth: the call's upload (tables | ring offsets | block images | rows) | every unit's stacks, points, flags, records
    DevBuf<unsigned char> d_depth;
    uint64_t next_gen = 1;
};

namespace {

constexpr size_t kFrDefaultArena = (1u << 20) / sizeof(int);   // words
constexpr size_t kFrAlign = 16;                                 // words: every block starts on a 64-byte line
constexpr size_t kFrDefaultRows = (1u << 20) / 64;              // rows

inline size_t fr_round(size_t words) { return (words + kFrAlign - 1) / kFrAlign * kFrAlign; }

// the units of a call cut into chunks of kFrChunk keypoints, unit after unit: unit u owns the chunks [chunk0[u], chunk0[u + 1])
struct FrChunks {
    std::vector<int> chunk0{0};
    int n_chunks = 0, max_chunks = 0;
    void add(int n) { max_chunks = std::max(max_chunks, cdiv(n, kFrChunk)); n_chunks += cdiv(n, kFrChunk); chunk0.push_back(n_chunks); }
    int of(int u) const { return chunk0[(size_t)u + 1] - chunk0[(size_t)u]; }
};

int fr_need_store(velo_ctx* c, const char* who) {
    if (!c->fr) return fail(VELO_ERR_STATE, "%s: velo_frames_reset has not run on this context", who);
    return VELO_OK;
}

void fr_side(const FrStore& S, const FrStore::Entry& e, FrSide* out) {
    const int* b = S.kp.at(e.blk);
    out->ids = b;
    out->has_depth = b + e.n;
    out->xy = reinterpret_cast<const float*>(b + 2 * (size_t)e.n);
    out->cloud = reinterpret_cast<const float*>(b + 4 * (size_t)e.n);
    out->n = e.n; out->pad = 0;
}

// The context's visual set indexes the entries of frame1 as they are now (velo_frames_prune asks): whatever replaces, prunes or
// drops an entry gives it a new stamp, velo_set_visual and velo_frames_reset forget the frame.
void fr_stamp_visual(velo_ctx* c, int frame1) {
    const FrStore& S = *c->fr;
    c->vis_frame1 = frame1;
    for (int cam = 0; cam < S.n_cams; cam++) c->vis_gen[cam] = S.dir.at(lm_key(frame1, cam)).gen;
}

// the state velo_set_visual leaves, for context i of a build call whose records are in vm: per_cam [n_cams] matches, pairs their
// (point1, point2) in record order; the host copy of the records holds what velo_get_good_matches reads
void fr_leave_visual(velo_ctx* c, int i, const int* per_cam, const int* pairs, int32_t* n_per_cam, int32_t* pairs_out, int32_t capacity,
                     int32_t* n_out) {
    velo_match zero;
    std::memset(&zero, 0, sizeof(zero));
    c->h_matches.clear();
    int total = 0;
    for (int cam = 0; cam < c->fr->n_cams; cam++) {
        const int m = per_cam[cam];
        if (n_per_cam) n_per_cam[(size_t)i * kLmMaxCams + cam] = m;
        for (int k = 0; k < m; k++) {
            const int* pr = pairs + 2 * ((size_t)total + (size_t)k);
            velo_match r = zero;
            r.cam = cam; r.point1 = pr[0]; r.point2 = pr[1];
            c->h_matches.push_back(r);
        }
        total += m;
    }
    c->n_matches = total;
    c->vflags_valid = false;
    c->h_vflags.clear();
    n_out[i] = total;
    const int w = std::min(total, (int)capacity);
    if (pairs_out && w > 0) std::memcpy(pairs_out + 2 * (size_t)i * capacity, pairs, sizeof(int32_t) * 2 * (size_t)w);
}

// room for a visual set of n records on context c
int fr_reserve_visual(velo_ctx* c, size_t n) {
    // records of an earlier velo_register_batch_visual may still be on their way into vm (set_visual_impl without a wait)
    if (c->pin[3].pending) { HIP_TRY(hipEventSynchronize(c->pin[3].ev)); c->pin[3].pending = false; }
    if (n > 0) {
        VELO_TRY(c->vm.reserve(n));
        VELO_TRY(c->vflags.reserve(3 * n));
    }
    return VELO_OK;
}

// context i of a call: where its records and their pairs go, and what the landmark substitution reads
void fr_fill_ctx(const velo_ctx* c, int i, int* d_pairs, const double* pose2_inv, FrCtx* K) {
    K->vm = c->vm.p;
    K->pairs = d_pairs;
    if (pose2_inv && c->lm && c->lm->n_ids > 0) {
        K->lm_pts = c->lm->pts.p; K->lm_added = c->lm->added.p; K->lm_ids = (int)c->lm->n_ids;
        std::memcpy(K->pose2_inv.m, pose2_inv + 16 * (size_t)i, sizeof(K->pose2_inv.m));
    }
}

int fr_clear_vflags(velo_ctx* c, size_t n, hipStream_t st) {
    if (n > 0) HIP_TRY(hipMemsetAsync(c->vflags.p, 0, 3 * n, st));
    return VELO_OK;
}

// what velo_build_matches_batch and velo_build_matches_desc_batch (match_thresh: its threshold, else null) check before any context is touched
int fr_check_build_args(velo_ctx** ctxs, int n_ctx, const int32_t* frames1, const int32_t* frames2, const double* pose2_inv,
                        const double* match_thresh, int32_t capacity, const int32_t* n_out) {
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    if (!frames1 || !frames2) return fail(VELO_ERR_INVALID, "null frames");
    if (!n_out) return fail(VELO_ERR_INVALID, "null n_out");
    if (capacity < 0) return fail(VELO_ERR_INVALID, "negative capacity");
    if (match_thresh && std::isnan(*match_thresh)) return fail(VELO_ERR_INVALID, "match_thresh is NaN");
    for (int i = 0; i < n_ctx; i++)
        for (int f : {frames1[i], frames2[i]}) VELO_TRY(check_frame(f, "context", i));
    if (pose2_inv)
        for (int k = 0; k < 16 * n_ctx; k++) if (!std::isfinite(pose2_inv[k])) return fail(VELO_ERR_INVALID, "context %d: pose2_inv[%d] is not finite", k / 16, k % 16);
    return fb_check_devices(ctxs, n_ctx);
}

int fr_build_run(velo_ctx** ctxs, int n_ctx, const int32_t* frames1, const int32_t* frames2, const double* pose2_inv, int32_t* n_per_cam,
                 int32_t* pairs_out, int32_t capacity, int32_t* n_out) {
    // state first: nothing changes when a frame is missing
    for (int i = 0; i < n_ctx; i++) {
        VELO_TRY(fr_need_store(ctxs[i], "velo_build_matches"));
        const FrStore& S = *ctxs[i]->fr;
        for (int cam = 0; cam < S.n_cams; cam++)
            for (int f : {frames1[i], frames2[i]})
                if (!S.dir.count(lm_key(f, cam))) return fail(VELO_ERR_STATE, "context %d: frame %d, camera %d has not been put", i, f, cam);
    }
    velo_ctx* c0 = ctxs[0];
    FrStore* L = c0->fr.get();
    HIP_TRY(hipSetDevice(c0->device));
    // the units of the call, context-major and camera-major, and every context's share of the outputs
    int n_units = 0, max_n1 = 0;
    size_t all_n2 = 0;
    std::vector<int> unit0(n_ctx + 1, 0);
    FrChunks ck;
    std::vector<size_t> pair0(n_ctx + 1, 0);
    for (int i = 0; i < n_ctx; i++) {
        const FrStore& S = *ctxs[i]->fr;
        for (int cam = 0; cam < S.n_cams; cam++) {
            const FrStore::Entry& e1 = S.dir.at(lm_key(frames1[i], cam));
            const FrStore::Entry& e2 = S.dir.at(lm_key(frames2[i], cam));
            ck.add(e2.n);
            max_n1 = std::max(max_n1, e1.n);
            all_n2 += (size_t)e2.n;
            n_units++;
        }
        unit0[i + 1] = n_units;
        pair0[i + 1] = all_n2;
    }
    // room: slot tables, the visual sets, the staging
    std::vector<char> refill(n_ctx, 0);
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* c = ctxs[i];
        FrStore& S = *c->fr;
        int max_id = -1;
        for (int cam = 0; cam < S.n_cams; cam++) max_id = std::max(max_id, S.dir.at(lm_key(frames1[i], cam)).max_id);
        if ((size_t)(max_id + 1) > S.slot_ids) {
            // the tables hold -1 everywhere between calls, so a larger one is filled, not copied
            const size_t ids = std::max<size_t>({(size_t)max_id + 1, 2 * S.slot_ids, 4096});
            S.slot_ids = 0;
            VELO_TRY(S.slots.reserve(ids * (size_t)S.n_cams));
            S.slot_ids = ids;
            S.slots_dirty = true;                                    // uninitialised until this call's fill is queued and the call ends well
        }
        if (S.slots_dirty) refill[i] = 1;
        VELO_TRY(fr_reserve_visual(c, pair0[i + 1] - pair0[i]));
    }
    StageLayout in, out;
    const auto units = in.add<FrUnit>((size_t)n_units);
    const auto kctx = in.add<FrCtx>((size_t)n_ctx);
    const auto counts = out.add<int>((size_t)ck.n_chunks);
    const auto pairs = out.add<int>(2 * all_n2);
    VELO_TRY(L->in.reserve(in.bytes));
    VELO_TRY(L->out.reserve(std::max<size_t>(out.bytes, 64)));
    int* d_counts = counts.in(L->out.d.p);
    int* d_pairs = pairs.in(L->out.d.p);
    {
        FrUnit* hu = units.in(L->in.h.p);
        FrCtx* hc = kctx.in(L->in.h.p);
        std::memset(L->in.h.p, 0, in.bytes);
        for (int i = 0; i < n_ctx; i++) {
            velo_ctx* c = ctxs[i];
            const FrStore& S = *c->fr;
            for (int cam = 0; cam < S.n_cams; cam++) {
                FrUnit& U = hu[unit0[i] + cam];
                fr_side(S, S.dir.at(lm_key(frames1[i], cam)), &U.f1);
                fr_side(S, S.dir.at(lm_key(frames2[i], cam)), &U.f2);
                U.slots = S.slots.p + (size_t)cam * S.slot_ids;
                U.slot_ids = (int)S.slot_ids;
                U.ctx = i; U.cam = cam;
                U.chunk0 = ck.chunk0[(size_t)(unit0[i] + cam)];
                U.ctx_chunk0 = ck.chunk0[(size_t)unit0[i]];
                for (int k = 0; k < 3; k++) U.t_cam[k] = S.cam_t[3 * cam + k];
            }
            fr_fill_ctx(c, i, d_pairs + 2 * pair0[i], pose2_inv, &hc[i]);
        }
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, nullptr));
    hipStream_t st = c0->stream;
    for (int i = 0; i < n_ctx; i++) {
        FrStore& S = *ctxs[i]->fr;
        if (refill[i] && S.slot_ids > 0) HIP_TRY(hipMemsetAsync(S.slots.p, 0xFF, sizeof(int) * S.slot_ids * (size_t)S.n_cams, st));
        S.slots_dirty = true;                                        // until the clear launch is known to have run
        VELO_TRY(fr_clear_vflags(ctxs[i], pair0[i + 1] - pair0[i], st));
    }
    HIP_TRY(hipMemcpyAsync(L->in.d.p, L->in.h.p, in.bytes, hipMemcpyHostToDevice, st));
    const FrUnit* d_units = units.in(L->in.d.p);
    const FrCtx* d_ctxs = kctx.in(L->in.d.p);
    if (ck.n_chunks > 0) {
        const dim3 g1((unsigned)std::max(cdiv(max_n1, 256), 1), (unsigned)n_units), g2((unsigned)ck.max_chunks, (unsigned)n_units);
        if (max_n1 > 0) hipLaunchKernelGGL(fr_fill_kernel, g1, dim3(256), 0, st, d_units);
        hipLaunchKernelGGL(fr_count_kernel, g2, dim3(kFrChunk), 0, st, d_units, d_counts);
        hipLaunchKernelGGL(fr_emit_kernel, g2, dim3(kFrChunk), 0, st, d_units, d_ctxs, (const int*)d_counts);
        if (max_n1 > 0) hipLaunchKernelGGL(fr_clear_kernel, g1, dim3(256), 0, st, d_units);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(L->out.h.p, L->out.d.p, out.bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    const int* h_counts = counts.in(L->out.h.p);
    const int* h_pairs = pairs.in(L->out.h.p);
    for (int i = 0; i < n_ctx; i++) {
        FrStore& S = *ctxs[i]->fr;
        S.slots_dirty = false;
        int per_cam[kLmMaxCams];
        for (int cam = 0; cam < S.n_cams; cam++) {
            const int u = unit0[i] + cam;
            per_cam[cam] = 0;
            for (int k = ck.chunk0[(size_t)u]; k < ck.chunk0[(size_t)u + 1]; k++) per_cam[cam] += h_counts[k];
        }
        fr_leave_visual(ctxs[i], i, per_cam, h_pairs + 2 * pair0[i], n_per_cam, pairs_out, capacity, n_out);
        fr_stamp_visual(ctxs[i], frames1[i]);
    }
    return VELO_OK;
}

void fr_free_rows(FrStore& S, int64_t key) {
    auto it = S.rdir.find(key);
    if (it == S.rdir.end()) return;
    S.rows.list.release(it->second.blk);
    S.rdir.erase(it);
}

// One launch set of descriptor matching on resident rows.  build: context i joins (frames1[i], frames2[i]) camera by camera and its
// visual set becomes the kept pairs' records (velo_build_matches_desc[_batch]); else the ONE context's frames1[0] is screened against
// the n_cand frames of frames2, job-major candidate, camera (velo_match_frames: kept / min_d, nothing else changes).
int fr_desc_run(velo_ctx** ctxs, int n_ctx, const int32_t* frames1, const int32_t* frames2, int n_cand, bool build, const double* pose2_inv,
                double match_thresh, int32_t* n_per_cam, int32_t* pairs_out, int32_t capacity, int32_t* n_out, int32_t* kept, int32_t* min_d) {
    const char* who = build ? "velo_build_matches_desc" : "velo_match_frames";
    // state first: nothing changes when a frame or its rows are missing
    for (int i = 0; i < n_ctx; i++) {
        VELO_TRY(fr_need_store(ctxs[i], who));
        const FrStore& S = *ctxs[i]->fr;
        const int n2 = build ? 1 : n_cand;
        for (int cam = 0; cam < S.n_cams; cam++)
            for (int k = -1; k < n2; k++) {
                const int f = k < 0 ? frames1[i] : frames2[build ? i : k];
                if (!S.dir.count(lm_key(f, cam))) return fail(VELO_ERR_STATE, "context %d: frame %d, camera %d has not been put", i, f, cam);
                if (!S.rdir.count(lm_key(f, cam))) return fail(VELO_ERR_STATE, "context %d: frame %d, camera %d has no descriptor rows", i, f, cam);
            }
    }
    velo_ctx* c0 = ctxs[0];
    FrStore* L = c0->fr.get();
    HIP_TRY(hipSetDevice(c0->device));
    // the jobs of the call: context-major (or candidate-major), camera-major; a build's job u is its unit u
    std::vector<MatchResJob> jobs;
    std::vector<int> unit0(n_ctx + 1, 0);
    std::vector<size_t> pair0(n_ctx + 1, 0);
    int64_t blocks = 0, total_q = 0;
    int max_nq = 0;
    for (int i = 0; i < n_ctx; i++) {
        const FrStore& S = *ctxs[i]->fr;
        for (int k = 0; k < (build ? 1 : n_cand); k++)
            for (int cam = 0; cam < S.n_cams; cam++) {
                const FrStore::RowEntry& r1 = S.rdir.at(lm_key(frames1[i], cam));
                const FrStore::RowEntry& r2 = S.rdir.at(lm_key(frames2[build ? i : k], cam));
                MatchResJob M;
                std::memset(&M, 0, sizeof(M));
                M.q = S.rows.at(r1.blk); M.t = S.rows.at(r2.blk);
                M.n_query = r1.n; M.n_train = r2.n;
                M.q_out = (int)total_q;
                M.blk_start = (int)blocks;
                M.nqb = cdiv(r1.n, kMatchQ);
                if (r1.n > 0 && r2.n > 0) blocks += (int64_t)M.nqb * cdiv(r2.n, kMatchT);
                total_q += r1.n;
                max_nq = std::max(max_nq, r1.n);
                jobs.push_back(M);
            }
        unit0[i + 1] = (int)jobs.size();
        pair0[i + 1] = (size_t)total_q;
    }
    if (total_q > (int64_t)(INT32_MAX / 4)) return fail(VELO_ERR_INVALID, "%lld queries in one call; at most %d", (long long)total_q, INT32_MAX / 4);
    if (blocks > (int64_t)INT32_MAX) return fail(VELO_ERR_INVALID, "too many match blocks in one call");
    const int n_jobs = (int)jobs.size(), nq = (int)total_q;
    // room: the visual sets, the staging
    if (build)
        for (int i = 0; i < n_ctx; i++) VELO_TRY(fr_reserve_visual(ctxs[i], pair0[i + 1] - pair0[i]));
    // device input: jobs | units | contexts; device output: the filter's four arrays, ONE part that the filter kernel lays out
    // itself (4 nq + 2 j) | the records' pairs, context after context, packed behind it
    StageLayout in, out;
    const auto mjobs = in.add<MatchResJob>((size_t)n_jobs);
    const auto units = in.add<FrDescUnit>(build ? (size_t)n_jobs : 0);
    const auto kctx = in.add<FrCtx>(build ? (size_t)n_ctx : 0);
    const auto filt = out.add<int>(4 * (size_t)nq + 2 * (size_t)n_jobs);
    const auto pairs = out.add<int>(build ? 2 * (size_t)nq : 0, 4);
    const size_t back_ints = 2 * (size_t)n_jobs + pairs.n;                               // {min_dist, n_kept} per job | pairs: what comes back
    VELO_TRY(L->in.reserve(in.bytes));
    VELO_TRY(L->out.h.reserve(sizeof(int) * back_ints));
    VELO_TRY(L->out.d.reserve(out.bytes));
    VELO_TRY(L->d_keys.reserve((size_t)nq + (size_t)n_jobs));
    int* d_filt = filt.in(L->out.d.p);
    int* d_job_out = d_filt + 4 * (size_t)nq;
    int* d_pairs = pairs.in(L->out.d.p);
    std::memset(L->in.h.p, 0, in.bytes);
    std::memcpy(mjobs.in(L->in.h.p), jobs.data(), mjobs.size());
    if (build) {
        FrDescUnit* hu = units.in(L->in.h.p);
        FrCtx* hc = kctx.in(L->in.h.p);
        for (int i = 0; i < n_ctx; i++) {
            velo_ctx* c = ctxs[i];
            const FrStore& S = *c->fr;
            for (int cam = 0; cam < S.n_cams; cam++) {
                FrDescUnit& U = hu[unit0[i] + cam];
                fr_side(S, S.dir.at(lm_key(frames1[i], cam)), &U.f1);
                fr_side(S, S.dir.at(lm_key(frames2[i], cam)), &U.f2);
                U.ctx = i; U.cam = cam;
                U.ctx_unit0 = unit0[i];
                U.q_out = jobs[(size_t)(unit0[i] + cam)].q_out;
                for (int k = 0; k < 3; k++) U.t_cam[k] = S.cam_t[3 * cam + k];
            }
            fr_fill_ctx(c, i, d_pairs + 2 * pair0[i], pose2_inv, &hc[i]);
        }
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, nullptr));
    hipStream_t st = c0->stream;
    if (build)
        for (int i = 0; i < n_ctx; i++) VELO_TRY(fr_clear_vflags(ctxs[i], pair0[i + 1] - pair0[i], st));
    if (n_jobs > 0) {
        HIP_TRY(hipMemcpyAsync(L->in.d.p, L->in.h.p, in.bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(L->d_keys.p, 0xFF, sizeof(unsigned) * ((size_t)nq + (size_t)n_jobs), st));   // kMatchNone
        const MatchResJob* d_jobs = mjobs.in(L->in.d.p);
        unsigned* keys = L->d_keys.p;
        unsigned* dmin = L->d_keys.p + nq;
        if (blocks > 0)
            hipLaunchKernelGGL(match_mfma_resident_kernel, dim3((unsigned)blocks), dim3(kMatchThreads), 0, st, d_jobs, n_jobs, keys, dmin);
        hipLaunchKernelGGL(match_filter_resident_kernel, dim3((unsigned)n_jobs), dim3(kMatchThreads), 0, st, d_jobs, (const unsigned*)keys,
                           (const unsigned*)dmin, match_thresh, nq, d_filt);
        if (build && max_nq > 0)
            hipLaunchKernelGGL(fr_emit_desc_kernel, dim3((unsigned)cdiv(max_nq, 256), (unsigned)n_jobs), dim3(256), 0, st,
                               (const FrDescUnit*)units.in(L->in.d.p), (const FrCtx*)kctx.in(L->in.d.p),
                               (const int*)d_job_out, (const int*)(d_filt + 2 * (size_t)nq));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(L->out.h.p, d_job_out, sizeof(int) * back_ints, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    const int* h_job = (const int*)L->out.h.p;
    if (!build) {
        for (int j = 0; j < n_jobs; j++) { min_d[j] = h_job[2 * j]; kept[j] = h_job[2 * j + 1]; }
        return VELO_OK;
    }
    const int* h_pairs = h_job + 2 * (size_t)n_jobs;
    for (int i = 0; i < n_ctx; i++) {
        int per_cam[kLmMaxCams];
        for (int cam = 0; cam < ctxs[i]->fr->n_cams; cam++) per_cam[cam] = h_job[2 * (unit0[i] + cam) + 1];
        fr_leave_visual(ctxs[i], i, per_cam, h_pairs + 2 * pair0[i], n_per_cam, pairs_out, capacity, n_out);
        fr_stamp_visual(ctxs[i], frames1[i]);
    }
    return VELO_OK;
}

// One launch set that cuts entries down to a keep set (velo.h:282-326 per entry).  keep_cam < 0: every camera of frames[i] of ctxs[i],
// the keep set read from the context's visual set and its gate flags (velo_frames_prune[_batch]; outputs [n_ctx][8], [n_ctx][capacity],
// [n_ctx]); else the ONE entry (frames[0], keep_cam) of the one context and the n_keep indices of keep_idx (velo_frames_keep; outputs
// of one entry).  The callers have checked the arguments; the state is checked here, before anything changes.
int fr_prune_run(velo_ctx** ctxs, int n_ctx, const int32_t* frames, int keep_cam, const int32_t* keep_idx, int32_t n_keep, int32_t* n_kept,
                 int32_t* n_with_depth, int32_t* kept_out, int32_t capacity, int32_t* n_out) {
    const bool by_list = keep_cam >= 0;
    const char* who = by_list ? "velo_frames_keep" : "velo_frames_prune";
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* c = ctxs[i];
        VELO_TRY(fr_need_store(c, who));
        const FrStore& S = *c->fr;
        if (by_list) {
            auto it = S.dir.find(lm_key(frames[i], keep_cam));
            if (it == S.dir.end()) return fail(VELO_ERR_STATE, "frame %d, camera %d has not been put", frames[i], keep_cam);
            for (int k = 0; k < n_keep; k++)
                if (keep_idx[k] < 0 || keep_idx[k] >= it->second.n)
                    return fail(VELO_ERR_INVALID, "keep_idx[%d] = %d; the entry has %d keypoints", k, keep_idx[k], it->second.n);
            continue;
        }
        for (int cam = 0; cam < S.n_cams; cam++)
            if (!S.dir.count(lm_key(frames[i], cam))) return fail(VELO_ERR_STATE, "context %d: frame %d, camera %d has not been put", i, frames[i], cam);
        if (c->vis_frame1 != frames[i])
            return fail(VELO_ERR_STATE, "context %d: the visual set was not built with frame %d as frame1 (velo_build_matches[_desc])", i, frames[i]);
        for (int cam = 0; cam < S.n_cams; cam++)
            if (c->vis_gen[cam] != S.dir.at(lm_key(frames[i], cam)).gen)
                return fail(VELO_ERR_STATE, "context %d: frame %d, camera %d has changed since the visual set was built from it", i, frames[i], cam);
        if (!c->vflags_valid) return fail(VELO_ERR_STATE, "context %d: no registration or velo_build_visual since the visual set was built", i);
        if (c->shard_world > 1) return fail(VELO_ERR_STATE, "context %d: rank %d of %d sweeps a slice of the visual set only", i, c->shard_rank, c->shard_world);
    }
    velo_ctx* c0 = ctxs[0];
    FrStore* L = c0->fr.get();
    HIP_TRY(hipSetDevice(c0->device));
    // the units of the call, context-major and camera-major, and where each one's share of the scratch and of the outputs lies
    struct Span { size_t map, out, rows, kept; };
    std::vector<FrStore::Entry*> ent;
    std::vector<FrStore::RowEntry*> rent;
    std::vector<Span> span;
    std::vector<int> unit0(n_ctx + 1, 0);
    FrChunks ck;
    StageLayout maps;                                                // every unit's keep map on a 64-byte line of its own
    size_t out_words = 0, row_count = 0, all_n = 0;
    int max_src = by_list ? (int)n_keep : 0;
    for (int i = 0; i < n_ctx; i++) {
        FrStore& S = *ctxs[i]->fr;
        for (int cam = by_list ? keep_cam : 0; cam < (by_list ? keep_cam + 1 : S.n_cams); cam++) {
            FrStore::Entry& e = S.dir.at(lm_key(frames[i], cam));
            auto r = S.rdir.find(lm_key(frames[i], cam));
            ent.push_back(&e);
            rent.push_back(r != S.rdir.end() ? &r->second : nullptr);
            span.push_back(Span{maps.add<unsigned char>((size_t)e.n).off, out_words, row_count, all_n});
            ck.add(e.n);
            out_words += fr_round(7 * (size_t)e.n);                  // at most n kept, every one with a depth point of its own
            if (r != S.rdir.end()) row_count += (size_t)e.n;
            all_n += (size_t)e.n;
        }
        unit0[i + 1] = (int)ent.size();
        if (!by_list) max_src = std::max(max_src, ctxs[i]->n_matches);
    }
    const int n_units = (int)ent.size();
    // device input: units | sources | the keep list; device output, copied back in one piece: the chunk counts | the kept indices
    StageLayout in, out, scratch;                                    // (the scratch: keep maps in whole lines | gathered blocks | gathered rows)
    const auto units = in.add<FrPruneUnit>((size_t)n_units);
    const auto srcs = in.add<FrPruneSrc>((size_t)n_ctx);
    const auto keep = in.add<int>((size_t)(by_list ? n_keep : 0));
    const auto counts = out.add<int>((size_t)ck.n_chunks);
    const auto kept = out.add<int>(all_n);
    const auto smap = scratch.add<unsigned char>(maps.align(64));
    const auto sblocks = scratch.add<int>(out_words);
    const auto srows = scratch.add<uint4>(4 * row_count);
    VELO_TRY(L->in.reserve(in.bytes));
    VELO_TRY(L->out.reserve(std::max<size_t>(out.bytes, 64)));
    if (scratch.bytes > L->d_prune.cap) {                               // geometric, and kept
        HIP_TRY(hipStreamSynchronize(c0->stream));                       // the copies of the call before may still read the old scratch
        VELO_TRY(L->d_prune.reserve(std::max(scratch.bytes, 2 * L->d_prune.cap)));
    }
    unsigned char* d_map = smap.in(L->d_prune.p);
    int* d_blocks = sblocks.in(L->d_prune.p);
    uint4* d_rows = srows.in(L->d_prune.p);
    int* d_counts = counts.in(L->out.d.p);
    int* d_kept = kept.in(L->out.d.p);
    {
        FrPruneUnit* hu = units.in(L->in.h.p);
        FrPruneSrc* hs = srcs.in(L->in.h.p);
        std::memset(L->in.h.p, 0, in.bytes);
        for (int i = 0; i < n_ctx; i++) {
            velo_ctx* c = ctxs[i];
            const FrStore& S = *c->fr;
            for (int u = unit0[i]; u < unit0[i + 1]; u++) {
                FrPruneUnit& U = hu[u];
                fr_side(S, *ent[u], &U.f);
                U.rows = rent[u] ? S.rows.at(rent[u]->blk) : nullptr;
                U.map = d_map + span[u].map;
                U.out = d_blocks + span[u].out;
                U.rows_out = d_rows + 4 * span[u].rows;
                U.kept = d_kept + span[u].kept;
                U.chunk0 = ck.chunk0[(size_t)u]; U.n_chunks = ck.of(u);
            }
            FrPruneSrc& R = hs[i];
            R.unit0 = unit0[i]; R.n_cams = unit0[i + 1] - unit0[i];
            if (by_list) {
                R.keep = keep.in(L->in.d.p); R.n = n_keep;
                if (n_keep > 0) std::memcpy(keep.in(L->in.h.p), keep_idx, keep.size());
            } else { R.vm = c->vm.p; R.vflags = c->vflags.p; R.n = c->n_matches; }
        }
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, nullptr));
    hipStream_t st = c0->stream;
    if (ck.n_chunks > 0) {
        HIP_TRY(hipMemcpyAsync(L->in.d.p, L->in.h.p, in.bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_map, 0, smap.size(), st));
        const FrPruneUnit* d_units = units.in(L->in.d.p);
        const dim3 g((unsigned)ck.max_chunks, (unsigned)n_units);
        if (max_src > 0)
            hipLaunchKernelGGL(fr_mark_kernel, dim3((unsigned)cdiv(max_src, 256), (unsigned)n_ctx), dim3(256), 0, st, d_units,
                               (const FrPruneSrc*)srcs.in(L->in.d.p));
        hipLaunchKernelGGL(fr_prune_count_kernel, g, dim3(kFrChunk), 0, st, d_units, d_counts);
        hipLaunchKernelGGL(fr_prune_move_kernel, g, dim3(kFrChunk), 0, st, d_units, (const int*)d_counts);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(L->out.h.p, L->out.d.p, out.bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // The host now knows every unit's new size: it places the block (in place unless shared depth points made the cloud longer than the
    // block holds) and queues the copies out of the scratch behind the launches -- the only writes into an arena.  A unit's directory
    // entry changes after the last call of that unit that can fail.
    const int* h_counts = counts.in(L->out.h.p);
    const int* h_kept = kept.in(L->out.h.p);
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* c = ctxs[i];
        FrStore& S = *c->fr;
        int total = 0;
        for (int u = unit0[i]; u < unit0[i + 1]; u++) {
            int m = 0, m_wd = 0;
            for (int k = ck.chunk0[(size_t)u]; k < ck.chunk0[(size_t)u + 1]; k++) { m += h_counts[k] & 0xffff; m_wd += h_counts[k] >> 16; }
            FrStore::Entry& e = *ent[u];
            const size_t words = 4 * (size_t)m + 3 * (size_t)m_wd;
            BlockList::Plan plan;
            // an arena that has to grow is copied on its context's stream: not before the copies this call has queued into it have landed
            if (S.kp.list.plan(&e.blk, fr_round(words)).grow_to > 0) HIP_TRY(hipStreamSynchronize(st));
            VELO_TRY(S.kp.place(c, &e.blk, fr_round(words), &plan));
            if (words > 0)
                HIP_TRY(hipMemcpyAsync(S.kp.at(plan.block), d_blocks + span[u].out, sizeof(int) * words, hipMemcpyDeviceToDevice, st));
            if (rent[u] && m > 0)                                      // m <= n rows: always in place
                HIP_TRY(hipMemcpyAsync(S.rows.at(rent[u]->blk), d_rows + 4 * span[u].rows, 64 * (size_t)m, hipMemcpyDeviceToDevice, st));
            S.kp.list.commit(plan, &e.blk);
            e.blk = plan.block; e.n = m; e.n_wd = m_wd; e.gen = S.next_gen++;      // max_id stays an upper bound: it only sizes the slot table
            if (rent[u]) rent[u]->n = m;
            const int slot = by_list ? 0 : i * kLmMaxCams + (u - unit0[i]);
            if (n_kept) n_kept[slot] = m;
            if (n_with_depth) n_with_depth[slot] = m_wd;
            if (kept_out)
                for (int k = 0; k < m && total + k < capacity; k++) kept_out[(size_t)i * capacity + (size_t)(total + k)] = h_kept[span[u].kept + (size_t)k];
            total += m;
        }
        if (n_out) n_out[i] = total;
    }
    return fb_release(ctxs, n_ctx);
}

// One launch set that puts frames[i] of ctxs[i] with the depth of its keypoints computed on the device (velo_frames_put_frame[_batch];
// cams [n_ctx][8], n_with_depth [n_ctx][8] or null).  The callers have checked the list; everything else is checked here, before
// anything changes.  What the call leaves per camera is what velo_project_lidar, velo_depth_association, velo_frames_put,
// velo_frames_put_descriptors and (VELO_PUT_OBSERVE) velo_landmarks_observe leave, the arenas' and the log's bookkeeping included.
int fr_put_frame_run(velo_ctx** ctxs, int n_ctx, const int32_t* frames, const int32_t* of_target, const velo_frame_cam* cams, double thresh,
                     int32_t flags, int32_t* n_with_depth) {
    const bool observe = (flags & VELO_PUT_OBSERVE) != 0;
    struct Span {
        const velo_frame_cam* K;
        size_t img, rows;                                            // bytes into the upload
        size_t pstack, vstack, ring_cnt, kp_point, flag, obs, obs_ids;   // bytes into the scratch behind it
        int max_id;
    };
    std::vector<Span> span;
    std::vector<int> unit0(n_ctx + 1, 0);
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* c = ctxs[i];
        VELO_TRY(fr_need_store(c, "velo_frames_put_frame"));
        const FrStore& S = *c->fr;
        for (int cam = 0; cam < S.n_cams; cam++) {
            const velo_frame_cam& K = cams[(size_t)i * kLmMaxCams + cam];
            if (K.n < 0) return fail(VELO_ERR_INVALID, "context %d, camera %d: negative count", i, cam);
            if (K.n > 0 && (!K.ids || !K.keypoints_xy)) return fail(VELO_ERR_INVALID, "context %d, camera %d: null ids / keypoints", i, cam);
            if (K.rows && K.n > kMatchMaxRows)
                return fail(VELO_ERR_INVALID, "context %d, camera %d: %d descriptor rows; the match key indexes at most %d", i, cam, K.n, kMatchMaxRows);
            int32_t max_id = -1;
            for (int k = 0; k < K.n; k++) {
                if (K.ids[k] < 0) return fail(VELO_ERR_INVALID, "context %d, camera %d, entry %d: negative id %d", i, cam, k, K.ids[k]);
                if (K.ids[k] >= kLmMaxId) return fail(VELO_ERR_INVALID, "context %d, camera %d, entry %d: id %d; below %d", i, cam, k, K.ids[k], kLmMaxId);
                max_id = std::max(max_id, K.ids[k]);
            }
            if (observe && K.n > 1) {   // an id twice in one camera: found in a sorted copy, as velo_landmarks_observe finds it
                std::vector<int32_t> sorted(K.ids, K.ids + K.n);
                std::sort(sorted.begin(), sorted.end());
                for (int k = 1; k < K.n; k++)
                    if (sorted[(size_t)k] == sorted[(size_t)k - 1])
                        return fail(VELO_ERR_INVALID, "context %d, camera %d: id %d appears twice", i, cam, sorted[(size_t)k]);
            }
            Span sp;
            std::memset(&sp, 0, sizeof(sp));
            sp.K = &K; sp.max_id = max_id;
            span.push_back(sp);
        }
        unit0[i + 1] = (int)span.size();
    }
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* c = ctxs[i];
        if (of_target[i] ? !c->have_target : !c->have_source)
            return fail(VELO_ERR_STATE, "context %d: no %s cloud loaded", i, of_target[i] ? "target" : "source");
        if (!observe) continue;
        VELO_TRY(lm_need_store(c, "velo_frames_put_frame (VELO_PUT_OBSERVE)"));
        if (c->lm->n_cams != c->fr->n_cams)
            return fail(VELO_ERR_STATE, "context %d: the landmark store has %d cameras, the frame store %d", i, c->lm->n_cams, c->fr->n_cams);
        for (int cam = 0; cam < c->fr->n_cams; cam++)
            if (c->lm->lists.count(lm_key(frames[i], cam)))
                return fail(VELO_ERR_INVALID, "context %d: frame %d, camera %d has been observed already", i, frames[i], cam);
    }
    velo_ctx* c0 = ctxs[0];
    FrStore* L = c0->fr.get();
    HIP_TRY(hipSetDevice(c0->device));
    // where everything lies: the upload (units | every context's ring offsets | every unit's block image | its rows) and, behind it in
    // the same device buffer, every unit's share of the scratch.  A unit without keypoints projects nothing and owns no scratch.
    const int n_units = (int)span.size();
    std::vector<int> n_rings(n_ctx, 0), n_pts(n_ctx, 0);
    FrChunks ck;
    std::vector<size_t> off_at(n_ctx, 0);
    StageLayout lay;                                                 // ONE device buffer: the upload and the scratch behind it, every part on a line of its own
    auto take = [&lay](size_t bytes) { return lay.add<unsigned char>(bytes).off; };
    const auto units = lay.add<FrDepthUnit>((size_t)n_units);
    for (int i = 0; i < n_ctx; i++) {
        const velo_ctx* c = ctxs[i];
        n_rings[i] = std::max((int)(of_target[i] ? c->T->h_tgt_off : c->h_src_off).size() - 1, 0);
        n_pts[i] = of_target[i] ? c->T->n_tgt : c->n_src;
        off_at[i] = take(sizeof(int) * ((size_t)n_rings[i] + 1));
    }
    for (Span& sp : span) sp.img = take(sizeof(int) * fr_round(7 * (size_t)sp.K->n));          // at most n depth points
    for (Span& sp : span) if (sp.K->rows && sp.K->n > 0) sp.rows = take(64 * (size_t)sp.K->n);
    const size_t in_bytes = lay.align(64);                           // what is uploaded: whole lines
    int max_n = 0, max_rings = 0;
    for (int i = 0; i < n_ctx; i++)
        for (int u = unit0[i]; u < unit0[i + 1]; u++) {
            Span& sp = span[(size_t)u];
            const size_t n = (size_t)sp.K->n;
            ck.add(sp.K->n);
            max_n = std::max(max_n, sp.K->n);
            if (n == 0) continue;
            max_rings = std::max(max_rings, n_rings[i]);
            sp.pstack = take(sizeof(float4) * (size_t)std::max(n_pts[i], 1));
            sp.vstack = take(sizeof(float4) * (size_t)std::max(n_pts[i], 1));
            sp.ring_cnt = take(sizeof(int) * (size_t)std::max(n_rings[i], 1));
            sp.kp_point = take(sizeof(float4) * n);
            sp.flag = take(sizeof(int) * n);
            if (observe) { sp.obs = take(sizeof(velo_tri_obs) * n); sp.obs_ids = take(sizeof(int) * n); }
        }
    const size_t all_bytes = lay.align(64);
    StageLayout out;
    const auto counts = out.add<int>((size_t)ck.n_chunks);
    VELO_TRY(L->in.h.reserve(in_bytes));
    VELO_TRY(L->out.reserve(std::max<size_t>(out.bytes, 64)));
    if (all_bytes > L->d_depth.cap) {                                   // geometric, and kept
        HIP_TRY(hipStreamSynchronize(c0->stream));                       // the copies of the call before may still read the old scratch
        VELO_TRY(L->d_depth.reserve(std::max(all_bytes, 2 * L->d_depth.cap)));
    }
    // room in the landmark stores: the id tables and the log, which grows as the calls per camera would have grown it (velo_landmarks_info
    // shows capacity and reallocations) -- in one step, and the store's own numbers change with the rest of its bookkeeping
    struct LogPlan { size_t need_ids = 0, log_cap = 0; int reallocs = 0; };
    std::vector<LogPlan> lp(n_ctx);
    for (int i = 0; observe && i < n_ctx; i++) {
        velo_ctx* c = ctxs[i];
        LmStore& M = *c->lm;
        int max_id = -1;
        size_t len = M.log_len, cap = M.log_cap;
        for (int u = unit0[i]; u < unit0[i + 1]; u++) {
            const size_t n = (size_t)span[(size_t)u].K->n;
            max_id = std::max(max_id, span[(size_t)u].max_id);
            if (len + n > cap) { cap = std::max(len + n, 2 * cap); lp[i].reallocs++; }
            len += n;
        }
        lp[i].need_ids = std::max(M.n_ids, (size_t)(max_id + 1));
        lp[i].log_cap = cap;
        if (lp[i].need_ids > M.id_cap) {
            const size_t ids = std::max<size_t>({lp[i].need_ids, 2 * M.id_cap, 4096});
            VELO_TRY(lm_regrow(c, &M.head, M.n_ids, ids, 0xFF));       // -1: no observation yet
            VELO_TRY(lm_regrow(c, &M.count, M.n_ids, ids, 0));
            VELO_TRY(lm_regrow(c, &M.pts, 3 * M.n_ids, 3 * ids, 0));
            VELO_TRY(lm_regrow(c, &M.added, M.n_ids, ids, 0));
            M.id_cap = std::min(std::min(M.head.cap, M.count.cap), std::min(M.pts.cap / 3, M.added.cap));
        }
        if (cap > M.log_cap && (M.log.cap < cap || M.prev.cap < cap)) {
            VELO_TRY(lm_regrow(c, &M.log, M.log_len, cap, 0));
            VELO_TRY(lm_regrow(c, &M.prev, M.log_len, cap, 0xFF));
        }
    }
    unsigned char* dev = L->d_depth.p;
    {
        FrDepthUnit* hu = units.in(L->in.h.p);
        std::memset(hu, 0, units.size());
        for (int i = 0; i < n_ctx; i++) {
            const velo_ctx* c = ctxs[i];
            const FrStore& S = *c->fr;
            const std::vector<int>& h_off = of_target[i] ? c->T->h_tgt_off : c->h_src_off;
            int* ho = (int*)(L->in.h.p + off_at[i]);
            ho[0] = 0;
            if (n_rings[i] > 0) std::memcpy(ho, h_off.data(), sizeof(int) * ((size_t)n_rings[i] + 1));
            for (int u = unit0[i]; u < unit0[i + 1]; u++) {
                const Span& sp = span[(size_t)u];
                const velo_frame_cam& K = *sp.K;
                const int cam = u - unit0[i];
                const size_t n = (size_t)K.n;
                FrDepthUnit& U = hu[u];
                U.n = K.n; U.frame = frames[i]; U.cam = cam;
                U.chunk0 = ck.chunk0[(size_t)u]; U.n_chunks = ck.of(u);
                U.image = (int*)(dev + sp.img);
                if (n == 0) continue;
                U.pts = (const float4*)(of_target[i] ? c->T->tgt.p : c->src.p);
                U.off = (const int*)(dev + off_at[i]);
                U.n_rings = n_rings[i];
                U.W.tx = S.cam_t[3 * cam]; U.W.ty = S.cam_t[3 * cam + 1]; U.W.tz = S.cam_t[3 * cam + 2];
                U.W.min_x = K.bounds[0]; U.W.max_x = K.bounds[1]; U.W.min_y = K.bounds[2]; U.W.max_y = K.bounds[3];
                U.pstack = (float4*)(dev + sp.pstack); U.vstack = (float4*)(dev + sp.vstack); U.ring_cnt = (int*)(dev + sp.ring_cnt);
                U.kp_point = (float4*)(dev + sp.kp_point); U.flag = (int*)(dev + sp.flag);
                if (observe) { U.obs = (velo_tri_obs*)(dev + sp.obs); U.obs_ids = (int*)(dev + sp.obs_ids); }
                int* img = (int*)(L->in.h.p + sp.img);               // has_depth and the cloud are the device's to write
                std::memcpy(img, K.ids, sizeof(int) * n);
                std::memcpy(img + 2 * n, K.keypoints_xy, sizeof(float) * 2 * n);
                if (K.rows) std::memcpy(L->in.h.p + sp.rows, K.rows, 64 * n);
            }
        }
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, nullptr));
    hipStream_t st = c0->stream;
    int* d_counts = counts.in(L->out.d.p);
    if (ck.n_chunks > 0) {
        HIP_TRY(hipMemcpyAsync(dev, L->in.h.p, in_bytes, hipMemcpyHostToDevice, st));
        const FrDepthUnit* d_units = units.in(dev);
        const dim3 g((unsigned)ck.max_chunks, (unsigned)n_units);
        if (max_rings > 0) hipLaunchKernelGGL(fr_depth_project_kernel, dim3((unsigned)max_rings, (unsigned)n_units), dim3(256), 0, st, d_units);
        hipLaunchKernelGGL(fr_depth_assoc_kernel, dim3((unsigned)cdiv(max_n, 4), (unsigned)n_units), dim3(256), 0, st, d_units, thresh);
        hipLaunchKernelGGL(fr_depth_count_kernel, g, dim3(kFrChunk), 0, st, d_units, d_counts);
        hipLaunchKernelGGL(fr_depth_write_kernel, g, dim3(kFrChunk), 0, st, d_units, (const int*)d_counts);
        if (observe) {
            hipLaunchKernelGGL(fr_depth_obs_kernel, g, dim3(256), 0, st, d_units);
            // the append runs unchanged, a camera at a time: two cameras of a context may hold the same id
            for (int i = 0; i < n_ctx; i++) {
                LmStore& M = *ctxs[i]->lm;
                size_t base = M.log_len;
                for (int u = unit0[i]; u < unit0[i + 1]; u++) {
                    const Span& sp = span[(size_t)u];
                    const int n = sp.K->n;
                    if (n > 0)
                        hipLaunchKernelGGL(lm_append_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, st, (const velo_tri_obs*)(dev + sp.obs),
                                           (const int*)(dev + sp.obs_ids), n, (int)base, M.log.p, M.prev.p, M.head.p, M.count.p);
                    base += (size_t)n;
                }
            }
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(L->out.h.p, L->out.d.p, out.bytes, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    // The host now knows every block's size: it places the blocks in camera order -- the keypoint block as velo_frames_put would, the row
    // block as velo_frames_put_descriptors after it -- on COPIES of the arenas' lists, queues the copies out of the scratch behind the
    // launches, and hands lists and directories back after the last call that can fail.
    const int* h_counts = counts.in(L->out.h.p);
    struct Change { int64_t key; FrStore::Entry e; bool has_rows; FrStore::RowEntry r; };
    struct Pending { BlockList kl, rl; std::vector<Change> ch; };
    std::vector<Pending> pend(n_ctx);
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* c = ctxs[i];
        FrStore& S = *c->fr;
        Pending& P = pend[(size_t)i];
        P.kl = S.kp.list; P.rl = S.rows.list;
        for (int u = unit0[i]; u < unit0[i + 1]; u++) {
            const Span& sp = span[(size_t)u];
            const int n = sp.K->n;
            int n_wd = 0;
            for (int k = ck.chunk0[(size_t)u]; k < ck.chunk0[(size_t)u + 1]; k++) n_wd += h_counts[k];
            const size_t words = 4 * (size_t)n + 3 * (size_t)n_wd;
            Change C;
            C.key = lm_key(frames[i], u - unit0[i]);
            auto old = S.dir.find(C.key);
            const Block* old_blk = old != S.dir.end() ? &old->second.blk : nullptr;
            BlockList::Plan plan;
            // an arena that has to grow is copied on its context's stream: not before the copies this call has queued into it have landed
            if (P.kl.plan(old_blk, fr_round(words)).grow_to > 0) HIP_TRY(hipStreamSynchronize(st));
            VELO_TRY(S.kp.place(c, &P.kl, old_blk, fr_round(words), &plan));
            if (words > 0) HIP_TRY(hipMemcpyAsync(S.kp.at(plan.block), dev + sp.img, sizeof(int) * words, hipMemcpyDeviceToDevice, st));
            P.kl.commit(plan, old_blk);
            C.e = FrStore::Entry{plan.block, n, n_wd, sp.max_id, 0};
            // the rows the entry held go with its keypoints; new ones take a block of their own
            auto old_rows = S.rdir.find(C.key);
            if (old_rows != S.rdir.end()) P.rl.release(old_rows->second.blk);
            C.has_rows = sp.K->rows != nullptr;
            if (C.has_rows) {
                if (P.rl.plan(nullptr, (size_t)n).grow_to > 0) HIP_TRY(hipStreamSynchronize(st));
                VELO_TRY(S.rows.place(c, &P.rl, nullptr, (size_t)n, &plan));
                if (n > 0) HIP_TRY(hipMemcpyAsync(S.rows.at(plan.block), dev + sp.rows, 64 * (size_t)n, hipMemcpyDeviceToDevice, st));
                P.rl.commit(plan, nullptr);
                C.r = FrStore::RowEntry{plan.block, n};
            }
            P.ch.push_back(C);
            if (n_with_depth) n_with_depth[(size_t)i * kLmMaxCams + (size_t)(u - unit0[i])] = n_wd;
        }
    }
    VELO_TRY(fb_release(ctxs, n_ctx));
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* c = ctxs[i];
        FrStore& S = *c->fr;
        Pending& P = pend[(size_t)i];
        S.kp.list = std::move(P.kl); S.rows.list = std::move(P.rl);
        for (Change& C : P.ch) {
            C.e.gen = S.next_gen++;
            S.dir[C.key] = C.e;
            if (C.has_rows) S.rdir[C.key] = C.r; else S.rdir.erase(C.key);
        }
        if (!observe) continue;
        // velo_landmarks_observe's bookkeeping, camera after camera
        LmStore& M = *c->lm;
        const int frame = frames[i];
        M.log_cap = lp[i].log_cap; M.log_reallocs += lp[i].reallocs;
        if ((size_t)frame >= M.frame_seen.size()) { M.frame_seen.resize((size_t)frame + 1, 0); M.pose_set.resize((size_t)frame + 1, 0); }
        M.n_ids = lp[i].need_ids;
        if (M.h_count.size() < M.n_ids) { M.h_count.resize(M.n_ids, 0); M.h_added.resize(M.n_ids, 0); }
        for (int u = unit0[i]; u < unit0[i + 1]; u++) {
            const velo_frame_cam& K = *span[(size_t)u].K;
            if (!M.frame_seen[(size_t)frame] && K.n > 0) { M.frame_seen[(size_t)frame] = 1; if (!M.pose_set[(size_t)frame]) M.n_missing++; }
            M.lists[lm_key(frame, u - unit0[i])].assign(K.ids, K.ids + K.n);
            for (int k = 0; k < K.n; k++) M.h_count[(size_t)K.ids[k]]++;
            M.log_len += (size_t)K.n;
        }
    }
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)
int velo_frames_reset(velo_ctx* c, int32_t n_cams, const float* cam_trans, int32_t arena_capacity) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n_cams < 1 || n_cams > kLmMaxCams) return fail(VELO_ERR_INVALID, "%d cameras; 1..%d", n_cams, kLmMaxCams);
    if (!cam_trans) return fail(VELO_ERR_INVALID, "null cam_trans");
    if (arena_capacity < 0) return fail(VELO_ERR_INVALID, "negative arena capacity");
    for (int k = 0; k < 3 * n_cams; k++) if (!std::isfinite(cam_trans[k])) return fail(VELO_ERR_INVALID, "cam_trans[%d] is not finite", k);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // nothing of the old store is in flight when it goes
    c->fr.reset();
    c->vis_frame1 = -1;                                 // whatever the visual set was built from is gone
    std::shared_ptr<FrStore> S = std::make_shared<FrStore>();
    S->n_cams = n_cams;
    std::memcpy(S->cam_t, cam_trans, sizeof(float) * 3 * (size_t)n_cams);
    const size_t want = arena_capacity > 0 ? fr_round(((size_t)arena_capacity + sizeof(int) - 1) / sizeof(int)) : kFrDefaultArena;
    VELO_TRY(S->kp.buf.reserve(want));
    S->kp.list.cap = want;                              // the buffer holds a little more; the arena reallocates at what was asked for
    const size_t want_rows = arena_capacity > 0 ? ((size_t)arena_capacity + 63) / 64 : kFrDefaultRows;   // the row arena starts at the same byte count
    VELO_TRY(S->rows.buf.reserve(4 * want_rows));
    S->rows.list.cap = want_rows;
    c->fr = S;
    return VELO_OK;
}

int velo_frames_put(velo_ctx* c, int32_t frame, int32_t cam, const int32_t* ids, const float* keypoints_xy, const int32_t* has_depth,
                    const float* kp_with_depth_xyz, int32_t n_with_depth, int32_t n) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    VELO_TRY(check_cam(cam, kLmMaxCams));
    if (n < 0 || n_with_depth < 0) return fail(VELO_ERR_INVALID, "negative count");
    if (n > 0 && (!ids || !keypoints_xy || !has_depth)) return fail(VELO_ERR_INVALID, "null ids / keypoints / has_depth");
    if (n_with_depth > 0 && !kp_with_depth_xyz) return fail(VELO_ERR_INVALID, "a cloud of %d points and a null pointer", n_with_depth);
    int32_t max_id = -1;
    for (int i = 0; i < n; i++) {
        if (ids[i] < 0) return fail(VELO_ERR_INVALID, "entry %d: negative id %d", i, ids[i]);
        if (ids[i] >= kLmMaxId) return fail(VELO_ERR_INVALID, "entry %d: id %d; below %d", i, ids[i], kLmMaxId);
        if (has_depth[i] < -1 || has_depth[i] >= n_with_depth)
            return fail(VELO_ERR_INVALID, "entry %d: has_depth %d outside the cloud of %d points", i, has_depth[i], n_with_depth);
        max_id = std::max(max_id, ids[i]);
    }
    VELO_TRY(fr_need_store(c, "velo_frames_put"));
    FrStore& S = *c->fr;
    if (cam >= S.n_cams) return fail(VELO_ERR_INVALID, "camera %d; the store has %d", cam, S.n_cams);
    HIP_TRY(hipSetDevice(c->device));
    const size_t words = 4 * (size_t)n + 3 * (size_t)n_with_depth, need = fr_round(words);
    const int64_t key = lm_key(frame, cam);
    auto old = S.dir.find(key);
    const Block* old_blk = old != S.dir.end() ? &old->second.blk : nullptr;
    // where the block goes: in place when it fits, else the first free block that is large enough, else the front of the arena
    BlockList::Plan plan;
    VELO_TRY(S.kp.place(c, old_blk, need, &plan));
    if (words > 0) {
        unsigned char* stage = nullptr;
        VELO_TRY(S.put_stage.acquire(sizeof(int) * words, &stage));
        int* h = (int*)stage;
        if (n > 0) {
            std::memcpy(h, ids, sizeof(int) * (size_t)n);
            std::memcpy(h + n, has_depth, sizeof(int) * (size_t)n);
            std::memcpy(h + 2 * (size_t)n, keypoints_xy, sizeof(float) * 2 * (size_t)n);
        }
        if (n_with_depth > 0) std::memcpy(h + 4 * (size_t)n, kp_with_depth_xyz, sizeof(float) * 3 * (size_t)n_with_depth);
        HIP_TRY(hipMemcpyAsync(S.kp.at(plan.block), h, sizeof(int) * words, hipMemcpyHostToDevice, c->stream));
        VELO_TRY(S.put_stage.sent(c->stream));
    }
    // the directory after the last call that can fail
    S.kp.list.commit(plan, old_blk);
    S.dir[key] = FrStore::Entry{plan.block, n, n_with_depth, max_id, S.next_gen++};
    fr_free_rows(S, key);                                            // the keypoints the rows belonged to are gone
    return VELO_OK;
}

int velo_frames_drop(velo_ctx* c, int32_t frame) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    VELO_TRY(fr_need_store(c, "velo_frames_drop"));
    FrStore& S = *c->fr;
    for (int cam = 0; cam < S.n_cams; cam++) {
        auto it = S.dir.find(lm_key(frame, cam));
        if (it == S.dir.end()) continue;
        S.kp.list.release(it->second.blk);
        S.dir.erase(it);
        fr_free_rows(S, lm_key(frame, cam));
    }
    return VELO_OK;
}

int velo_frames_put_descriptors(velo_ctx* c, int32_t frame, int32_t cam, const uint8_t* rows, int32_t n) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    VELO_TRY(check_cam(cam, kLmMaxCams));
    if (n < 0) return fail(VELO_ERR_INVALID, "negative count");
    if (n > 0 && !rows) return fail(VELO_ERR_INVALID, "null descriptor rows");
    if (n > kMatchMaxRows) return fail(VELO_ERR_INVALID, "%d descriptor rows; the match key indexes at most %d", n, kMatchMaxRows);
    VELO_TRY(fr_need_store(c, "velo_frames_put_descriptors"));
    FrStore& S = *c->fr;
    const int64_t key = lm_key(frame, cam);
    auto kp = S.dir.find(key);
    if (kp == S.dir.end()) return fail(VELO_ERR_STATE, "frame %d, camera %d has not been put", frame, cam);
    if (n != kp->second.n) return fail(VELO_ERR_INVALID, "%d descriptor rows for the %d keypoints of frame %d, camera %d", n, kp->second.n, frame, cam);
    HIP_TRY(hipSetDevice(c->device));
    const size_t need = (size_t)n;
    auto old = S.rdir.find(key);
    const Block* old_blk = old != S.rdir.end() ? &old->second.blk : nullptr;
    BlockList::Plan plan;
    VELO_TRY(S.rows.place(c, old_blk, need, &plan));
    if (n > 0) {
        unsigned char* stage = nullptr;
        VELO_TRY(S.rows_stage.acquire(64 * need, &stage));
        std::memcpy(stage, rows, 64 * need);
        HIP_TRY(hipMemcpyAsync(S.rows.at(plan.block), stage, 64 * need, hipMemcpyHostToDevice, c->stream));
        VELO_TRY(S.rows_stage.sent(c->stream));
    }
    // the directory after the last call that can fail
    S.rows.list.commit(plan, old_blk);
    S.rdir[key] = FrStore::RowEntry{plan.block, n};
    return VELO_OK;
}

int velo_frames_desc_info(velo_ctx* c, int32_t* info) {
    if (!c || !info) return fail(VELO_ERR_INVALID, "null argument");
    VELO_TRY(fr_need_store(c, "velo_frames_desc_info"));
    const FrStore& S = *c->fr;
    info[0] = (int32_t)S.rdir.size(); info[1] = (int32_t)std::min<size_t>(S.rows.list.cap * 64, 0x7fffffff); info[2] = S.rows.list.reallocs;
    info[3] = (int32_t)S.rows.list.free_blocks.size();
    return VELO_OK;
}

int velo_frames_count(velo_ctx* c, int32_t frame, int32_t* n_per_cam, int32_t* n_total) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    VELO_TRY(fr_need_store(c, "velo_frames_count"));
    const FrStore& S = *c->fr;
    int total = 0;
    for (int cam = 0; cam < S.n_cams; cam++) {
        auto it = S.dir.find(lm_key(frame, cam));
        const int n = it == S.dir.end() ? -1 : it->second.n;
        if (n_per_cam) n_per_cam[cam] = n;
        total += std::max(n, 0);
    }
    if (n_total) *n_total = total;
    return VELO_OK;
}

int velo_frames_info(velo_ctx* c, int32_t* info) {
    if (!c || !info) return fail(VELO_ERR_INVALID, "null argument");
    VELO_TRY(fr_need_store(c, "velo_frames_info"));
    const FrStore& S = *c->fr;
    auto sat = [](size_t v) { return (int32_t)std::min<size_t>(v, 0x7fffffff); };    // an arena of 2 GiB or more reads as 2^31 - 1
    std::vector<int> frames;
    for (const auto& kv : S.dir) frames.push_back((int)(kv.first / kLmMaxCams));
    std::sort(frames.begin(), frames.end());
    frames.erase(std::unique(frames.begin(), frames.end()), frames.end());
    info[0] = (int32_t)frames.size(); info[1] = (int32_t)S.dir.size(); info[2] = sat(S.kp.list.cap * sizeof(int)); info[3] = S.kp.list.reallocs;
    info[4] = sat(S.kp.list.used * sizeof(int)); info[5] = S.n_cams; info[6] = (int32_t)S.slot_ids; info[7] = (int32_t)S.kp.list.free_blocks.size();
    return VELO_OK;
}

int velo_build_matches_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames1, const int32_t* frames2, const double* pose2_inv,
                             int32_t* n_per_cam, int32_t* pairs_out, int32_t capacity, int32_t* n_out) {
    VELO_TRY(fr_check_build_args(ctxs, n_ctx, frames1, frames2, pose2_inv, nullptr, capacity, n_out));
    return fr_build_run(ctxs, n_ctx, frames1, frames2, pose2_inv, n_per_cam, pairs_out, capacity, n_out);
}

int velo_build_matches(velo_ctx* c, int32_t frame1, int32_t frame2, const double* pose2_inv16, int32_t* n_per_cam, int32_t* pairs_out,
                       int32_t capacity, int32_t* n_out) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    return velo_build_matches_batch(&c, 1, &frame1, &frame2, pose2_inv16, n_per_cam, pairs_out, capacity, n_out);
}

int velo_build_matches_desc_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames1, const int32_t* frames2, const double* pose2_inv,
                                  double match_thresh, int32_t* n_per_cam, int32_t* pairs_out, int32_t capacity, int32_t* n_out) {
    VELO_TRY(fr_check_build_args(ctxs, n_ctx, frames1, frames2, pose2_inv, &match_thresh, capacity, n_out));
    return fr_desc_run(ctxs, n_ctx, frames1, frames2, 0, true, pose2_inv, match_thresh, n_per_cam, pairs_out, capacity, n_out, nullptr, nullptr);
}

int velo_build_matches_desc(velo_ctx* c, int32_t frame1, int32_t frame2, const double* pose2_inv16, double match_thresh, int32_t* n_per_cam,
                            int32_t* pairs_out, int32_t capacity, int32_t* n_out) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    return velo_build_matches_desc_batch(&c, 1, &frame1, &frame2, pose2_inv16, match_thresh, n_per_cam, pairs_out, capacity, n_out);
}

int velo_match_frames(velo_ctx* c, int32_t frame1, const int32_t* frames2, int32_t n_cand, double match_thresh, int32_t* n_kept,
                      int32_t* min_dist) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n_cand < 0) return fail(VELO_ERR_INVALID, "negative candidate count %d", n_cand);
    if (std::isnan(match_thresh)) return fail(VELO_ERR_INVALID, "match_thresh is NaN");
    VELO_TRY(check_frame(frame1));
    if (n_cand == 0) return VELO_OK;
    if (!frames2 || !n_kept || !min_dist) return fail(VELO_ERR_INVALID, "null frames2 / n_kept / min_dist");
    for (int k = 0; k < n_cand; k++) VELO_TRY(check_frame(frames2[k], "candidate", k));
    return fr_desc_run(&c, 1, &frame1, frames2, n_cand, false, nullptr, match_thresh, nullptr, nullptr, 0, nullptr, n_kept, min_dist);
}

int velo_frames_get(velo_ctx* c, int32_t frame, int32_t cam, int32_t* ids, float* keypoints_xy, int32_t* has_depth, float* kp_with_depth_xyz,
                    uint8_t* rows, int32_t capacity, int32_t capacity_with_depth, int32_t* n, int32_t* n_with_depth, int32_t* has_rows) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    VELO_TRY(check_cam(cam, kLmMaxCams));
    if (capacity < 0 || capacity_with_depth < 0) return fail(VELO_ERR_INVALID, "negative capacity");
    VELO_TRY(fr_need_store(c, "velo_frames_get"));
    const FrStore& S = *c->fr;
    auto it = S.dir.find(lm_key(frame, cam));
    if (it == S.dir.end()) return fail(VELO_ERR_STATE, "frame %d, camera %d has not been put", frame, cam);
    const FrStore::Entry& e = it->second;
    auto r = S.rdir.find(lm_key(frame, cam));
    if (n) *n = e.n;
    if (n_with_depth) *n_with_depth = e.n_wd;
    if (has_rows) *has_rows = r != S.rdir.end() ? 1 : 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // the uploads and the copies of a prune are queued there
    const size_t w = (size_t)std::min(e.n, (int)capacity), wd = (size_t)std::min(e.n_wd, (int)capacity_with_depth);
    const int* b = S.kp.at(e.blk);
    if (ids && w > 0) HIP_TRY(hipMemcpy(ids, b, sizeof(int) * w, hipMemcpyDeviceToHost));
    if (has_depth && w > 0) HIP_TRY(hipMemcpy(has_depth, b + e.n, sizeof(int) * w, hipMemcpyDeviceToHost));
    if (keypoints_xy && w > 0) HIP_TRY(hipMemcpy(keypoints_xy, b + 2 * (size_t)e.n, sizeof(float) * 2 * w, hipMemcpyDeviceToHost));
    if (kp_with_depth_xyz && wd > 0) HIP_TRY(hipMemcpy(kp_with_depth_xyz, b + 4 * (size_t)e.n, sizeof(float) * 3 * wd, hipMemcpyDeviceToHost));
    if (rows && r != S.rdir.end() && w > 0) HIP_TRY(hipMemcpy(rows, S.rows.at(r->second.blk), 64 * w, hipMemcpyDeviceToHost));
    return VELO_OK;
}

int velo_frames_keep(velo_ctx* c, int32_t frame, int32_t cam, const int32_t* keep_idx, int32_t n_keep, int32_t* kept_out, int32_t capacity,
                     int32_t* n_kept, int32_t* n_with_depth) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(check_frame(frame));
    VELO_TRY(check_cam(cam, kLmMaxCams));
    if (n_keep < 0 || capacity < 0) return fail(VELO_ERR_INVALID, "negative count");
    if (n_keep > 0 && !keep_idx) return fail(VELO_ERR_INVALID, "a keep list of %d indices and a null pointer", n_keep);
    return fr_prune_run(&c, 1, &frame, cam, keep_idx, n_keep, n_kept, n_with_depth, kept_out, capacity, nullptr);
}

int velo_frames_prune_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames, int32_t* n_kept, int32_t* n_with_depth, int32_t* kept_out,
                            int32_t capacity, int32_t* n_out) {
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    if (!frames) return fail(VELO_ERR_INVALID, "null frames");
    if (capacity < 0) return fail(VELO_ERR_INVALID, "negative capacity");
    for (int i = 0; i < n_ctx; i++) VELO_TRY(check_frame(frames[i], "context", i));
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    return fr_prune_run(ctxs, n_ctx, frames, -1, nullptr, 0, n_kept, n_with_depth, kept_out, capacity, n_out);
}

int velo_frames_prune(velo_ctx* c, int32_t frame, int32_t* n_kept, int32_t* n_with_depth, int32_t* kept_out, int32_t capacity, int32_t* n_out) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    return velo_frames_prune_batch(&c, 1, &frame, n_kept, n_with_depth, kept_out, capacity, n_out);
}

int velo_frames_put_frame_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames, const int32_t* of_target, const velo_frame_cam* cams,
                                double depth_assoc_thresh, int32_t flags, int32_t* n_with_depth) {
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    if (!frames || !of_target) return fail(VELO_ERR_INVALID, "null frames / of_target");
    if (!cams) return fail(VELO_ERR_INVALID, "null cams");
    if (flags & ~VELO_PUT_OBSERVE) return fail(VELO_ERR_INVALID, "unknown flags 0x%x", (unsigned)flags);
    for (int i = 0; i < n_ctx; i++) VELO_TRY(check_frame(frames[i], "context", i));
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    return fr_put_frame_run(ctxs, n_ctx, frames, of_target, cams, depth_assoc_thresh, flags, n_with_depth);
}

int velo_frames_put_frame(velo_ctx* c, int32_t frame, int32_t of_target, const velo_frame_cam* cams, double depth_assoc_thresh, int32_t flags,
                          int32_t* n_with_depth) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    return velo_frames_put_frame_batch(&c, 1, &frame, &of_target, cams, depth_assoc_thresh, flags, n_with_depth);
}

int velo_get_visual(velo_ctx* c, velo_match* out, int32_t capacity, int32_t* n) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (!n) return fail(VELO_ERR_INVALID, "null n");
    if (capacity < 0) return fail(VELO_ERR_INVALID, "negative capacity");
    *n = c->n_matches;
    const int w = std::min(c->n_matches, (int)capacity);
    if (!out || w <= 0) return VELO_OK;
    HIP_TRY(hipSetDevice(c->device));
    if (c->pin[3].pending) { HIP_TRY(hipEventSynchronize(c->pin[3].ev)); c->pin[3].pending = false; }   // records still on their way (set_visual_impl without a wait)
    HIP_TRY(hipStreamSynchronize(c->stream));
    static_assert(sizeof(VisualMatch) == sizeof(velo_match), "device/host match layout");
    HIP_TRY(hipMemcpy(out, c->vm.p, sizeof(velo_match) * (size_t)w, hipMemcpyDeviceToHost));
    return VELO_OK;
}

}  // extern "C"
