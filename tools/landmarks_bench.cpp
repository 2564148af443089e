// Driver of tools/landmarks_bench.py: walks n_ctx synthetic drives frame by frame through ONE of
//   a  the parent path: the reference's containers on the host (keypoint_obs2 / keypoint_obs3 / keypoint_obs_count, main.cpp:614-657)
//      plus velo_hip::triangulatePoints (the stateless velo_triangulate_points), one call per context
//   b  the resident store: LandmarkStore::setPose / observeFrame / triangulateFrame, one call per context
//   c  the resident store with ONE velo_landmarks_triangulate_batch call for all contexts
// and prints, for every frame count asked for, the host time of that frame's step (all contexts; the median of the 5 frames that end
// there).  `per_frame` landmarks are seen by both cameras in every frame and live `life` frames, so the accumulated log grows while
// a frame's work stays the same.  Usage: landmarks_bench MODE N_CTX PER_FRAME LIFE FRAME [FRAME ...]
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <vector>

#include "standins.hpp"
#include "velo_frame_to_frame.hpp"
#include "velo_landmarks.hpp"

typedef std::vector<std::vector<std::vector<standin::Point2f> > > Keypoints;      // [cam][frame][i]
typedef std::vector<std::vector<std::vector<int> > > Ints;
typedef std::vector<std::vector<standin::PointCloud::Ptr> > Clouds;

static unsigned g_seed = 12345u;
static double urand() { g_seed = g_seed * 1664525u + 1013904223u; return (g_seed >> 8) * (1.0 / 16777216.0); }

struct Drive {
    Keypoints keypoints; Ints keypoint_ids, has_depth; Clouds kp_with_depth;
    std::vector<std::array<double, 6> > poses;
    // path a
    std::vector<std::vector<std::map<int, standin::Point2f> > > obs2;
    std::vector<std::vector<std::map<int, standin::PointXYZ> > > obs3;
    std::vector<int> obs_count;
    std::vector<bool> added;
    standin::PointCloud::Ptr landmarks;
    std::unique_ptr<velo_hip::Context> ctx;
    std::unique_ptr<velo_hip::LandmarkStore> store;
};

static void make_frame(Drive& D, int frame, int per_frame, int life, const velo_hip::Rig& rig) {
    std::array<double, 6> pose = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.3 * frame}};
    D.poses.push_back(pose);
    const int first = (int)((long long)frame * per_frame / life);
    for (int cam = 0; cam < 2; cam++) {
        D.keypoints[cam].push_back(std::vector<standin::Point2f>()); D.keypoint_ids[cam].push_back(std::vector<int>());
        D.has_depth[cam].push_back(std::vector<int>()); D.kp_with_depth[cam].push_back(standin::PointCloud::Ptr(new standin::PointCloud));
        for (int k = 0; k < per_frame; k++) {
            const int id = first + k;
            unsigned h = (unsigned)id * 2654435761u;                 // the landmark's position follows from its id
            const double z = 8.0 + 30.0 * ((h >> 8) & 0xffff) / 65536.0 + 0.3 * ((double)id * life / per_frame);
            const double x = (((h >> 3) & 0xfff) / 4096.0 - 0.5) * 12.0, y = (((h >> 17) & 0xfff) / 4096.0 - 0.5) * 4.0;
            const double mz = z - pose[5];
            standin::Point2f p;
            p.x = (float)((x + rig.cam_trans[cam][0]) / mz + 7e-4 * (urand() - 0.5)); p.y = (float)(y / mz + 7e-4 * (urand() - 0.5));
            D.keypoints[cam][frame].push_back(p);
            D.keypoint_ids[cam][frame].push_back(id);
            if (cam == 0 && urand() < 0.3) {
                D.has_depth[cam][frame].push_back((int)D.kp_with_depth[cam][frame]->size());
                D.kp_with_depth[cam][frame]->push_back(standin::PointXYZ((float)(x + 0.03 * (urand() - 0.5)), (float)(y + 0.03 * (urand() - 0.5)), (float)(mz + 0.03 * (urand() - 0.5))));
            } else D.has_depth[cam][frame].push_back(-1);
        }
    }
}

// main.cpp:614-657 on the host; returns the ids to triangulate
static std::vector<int> host_bookkeeping(Drive& D, int frame) {
    int id_counter = (int)D.added.size() - 1;
    for (int cam = 0; cam < 2; cam++) for (int id : D.keypoint_ids[cam][frame]) id_counter = std::max(id_counter, id);
    D.added.resize(id_counter + 1, false);
    D.landmarks->points.resize(id_counter + 1);
    D.obs_count.resize(id_counter + 1, 0);
    D.obs2.resize(id_counter + 1, std::vector<std::map<int, standin::Point2f> >(2));
    D.obs3.resize(id_counter + 1, std::vector<std::map<int, standin::PointXYZ> >(2));
    for (int cam = 0; cam < 2; cam++)
        for (size_t i = 0; i < D.keypoints[cam][frame].size(); i++) {
            const int id = D.keypoint_ids[cam][frame][i];
            D.obs_count[id]++;
            if (D.has_depth[cam][frame][i] == -1) D.obs2[id][cam][frame] = D.keypoints[cam][frame][i];
            else D.obs3[id][cam][frame] = D.kp_with_depth[cam][frame]->at(D.has_depth[cam][frame][i]);
        }
    std::vector<int> ids;
    for (int cam = 0; cam < 2; cam++) ids.insert(ids.end(), D.keypoint_ids[cam][frame].begin(), D.keypoint_ids[cam][frame].end());
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    std::vector<int> out;
    for (int id : ids) if (D.obs_count[id] >= 3) out.push_back(id);
    return out;
}

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: landmarks_bench a|b|c n_ctx per_frame life frame [frame ...]\n"); return 2; }
    const char mode = argv[1][0];
    const int n_ctx = atoi(argv[2]), per_frame = atoi(argv[3]), life = atoi(argv[4]);
    std::vector<int> marks;
    for (int k = 5; k < argc; k++) marks.push_back(atoi(argv[k]));
    const int F = *std::max_element(marks.begin(), marks.end());
    velo_hip::Rig rig;
    std::vector<float> ct;
    for (int cam = 0; cam < 2; cam++) for (int k = 0; k < 3; k++) ct.push_back(rig.cam_trans[cam][k]);
    std::vector<Drive> drives(n_ctx);
    std::vector<velo_ctx*> handles;
    for (Drive& D : drives) {
        D.keypoints.resize(2); D.keypoint_ids.resize(2); D.has_depth.resize(2); D.kp_with_depth.resize(2);
        D.landmarks.reset(new standin::PointCloud);
        D.ctx.reset(new velo_hip::Context(0));
        if (mode != 'a') D.store.reset(new velo_hip::LandmarkStore(D.ctx->get(), 2, ct.data()));
        handles.push_back(D.ctx->get());
    }
    std::vector<double> us((size_t)F, 0.0);
    std::vector<int32_t> frames(n_ctx), n_out(n_ctx), ids_out;
    std::vector<float> pts_out;
    std::vector<velo_tri_result> res_out;
    long long solved = 0;
    for (int f = 0; f < F; f++) {
        for (Drive& D : drives) make_frame(D, f, per_frame, life, rig);          // the frame's inputs exist before the clock starts
        const auto t0 = std::chrono::steady_clock::now();
        if (mode == 'a') {
            for (Drive& D : drives) {
                const std::vector<int> ids = host_bookkeeping(D, f);
                velo_hip::triangulatePoints(*D.ctx, rig, ids, D.obs2, D.obs3, D.poses, (int)D.poses.size(), D.landmarks, D.added);
                for (int id : ids) D.added[id] = true;
                solved += (long long)ids.size();
            }
        } else {
            for (Drive& D : drives) {
                velo_hip::check(D.store->setPose(f, D.poses[f].data()), "setPose");
                velo_hip::check(D.store->observeFrame(f, D.keypoints, D.keypoint_ids, D.has_depth, D.kp_with_depth), "observeFrame");
                if (mode == 'b') {
                    std::vector<int> ids;
                    velo_hip::check(D.store->triangulateFrame(f, D.landmarks, D.added, &ids), "triangulateFrame");
                    solved += (long long)ids.size();
                }
            }
            if (mode == 'c') {
                int32_t cap = 1;
                for (int i = 0; i < n_ctx; i++) {
                    int32_t m = 0;
                    frames[i] = f;
                    velo_hip::check(velo_landmarks_frame_count(handles[i], f, 0, &m), "frame_count");
                    cap = std::max(cap, m);
                }
                ids_out.resize((size_t)n_ctx * cap); pts_out.resize((size_t)3 * n_ctx * cap); res_out.resize((size_t)n_ctx * cap);
                velo_hip::check(velo_landmarks_triangulate_batch(handles.data(), n_ctx, frames.data(), ids_out.data(), pts_out.data(), res_out.data(), cap,
                                                                 n_out.data()), "triangulate_batch");
                for (int i = 0; i < n_ctx; i++) {
                    Drive& D = drives[i];
                    int32_t info[8];
                    velo_hip::check(velo_landmarks_info(handles[i], info), "info");
                    if (D.landmarks->points.size() < (size_t)info[0]) { D.landmarks->points.resize(info[0]); D.added.resize(info[0], false); }
                    for (int32_t k = 0; k < n_out[i]; k++) {
                        const int id = ids_out[(size_t)i * cap + k];
                        standin::PointXYZ& p = D.landmarks->points[id];
                        p.x = pts_out[3 * ((size_t)i * cap + k)]; p.y = pts_out[3 * ((size_t)i * cap + k) + 1]; p.z = pts_out[3 * ((size_t)i * cap + k) + 2];
                        D.added[id] = true;
                    }
                    solved += n_out[i];
                }
            }
        }
        us[(size_t)f] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    }
    for (int m : marks) {
        std::vector<double> w(us.begin() + std::max(0, m - 5), us.begin() + m);
        std::sort(w.begin(), w.end());
        printf("step mode=%c n_ctx=%d frames=%d us=%.1f\n", mode, n_ctx, m, w[w.size() / 2]);
    }
    // a checksum of the last frame's landmarks, so that the three modes can be compared
    unsigned long long sum = 0;
    for (const Drive& D : drives) for (size_t id = 0; id < D.added.size(); id++) if (D.added[id]) { unsigned u; memcpy(&u, &D.landmarks->points[id].x, 4); sum = sum * 1099511628211ull + u; }
    printf("done mode=%c n_ctx=%d solved=%lld checksum=%016llx\n", mode, n_ctx, solved, sum);
    return 0;
}
