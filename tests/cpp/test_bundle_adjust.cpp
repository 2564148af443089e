// Driver of LandmarkStore::bundleAdjust (include/velo_landmarks.hpp) against stand-in container types: reads a sequence (cameras,
// poses, per frame and camera the keypoints, ids, has_depth and the depth cloud), walks it like main.cpp:614-679, bundle-adjusts the
// window of all frames and prints the summary, the poses as double bit patterns and the landmarks as float bit patterns.  Without an
// argument it only has to compile and link.
#include <cstdio>
#include <cstring>
#include <vector>

#include "standins.hpp"
#include "velo_landmarks.hpp"

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }
static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) { printf("bundle adjust adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int num_cams = 0, F = 0, n_fixed = 0;
    if (!rd(f, &num_cams, 1) || !rd(f, &F, 1) || !rd(f, &n_fixed, 1)) return 2;
    std::vector<float> cam_trans(3 * num_cams);
    std::vector<double> flat(6 * (size_t)F);
    if (!rd(f, &cam_trans[0], cam_trans.size()) || !rd(f, &flat[0], flat.size())) return 2;
    std::vector<std::vector<double> > ceres_poses_vec(F, std::vector<double>(6));
    for (int fr = 0; fr < F; fr++) for (int j = 0; j < 6; j++) ceres_poses_vec[fr][j] = flat[6 * (size_t)fr + j];
    std::vector<std::vector<std::vector<standin::Point2f> > > keypoints(num_cams, std::vector<std::vector<standin::Point2f> >(F));
    std::vector<std::vector<std::vector<int> > > keypoint_ids(num_cams, std::vector<std::vector<int> >(F)), has_depth(keypoint_ids);
    std::vector<std::vector<standin::PointCloud::Ptr> > kp_with_depth(num_cams, std::vector<standin::PointCloud::Ptr>(F));
    for (int fr = 0; fr < F; fr++)
        for (int cam = 0; cam < num_cams; cam++) {
            int n = 0, m = 0;
            if (!rd(f, &n, 1)) return 2;
            std::vector<float> xy(2 * (size_t)n);
            keypoint_ids[cam][fr].resize(n); has_depth[cam][fr].resize(n); keypoints[cam][fr].resize(n);
            if (!rd(f, keypoint_ids[cam][fr].data(), n) || !rd(f, xy.data(), xy.size()) || !rd(f, has_depth[cam][fr].data(), n) || !rd(f, &m, 1)) return 2;
            for (int i = 0; i < n; i++) { keypoints[cam][fr][i].x = xy[2 * i]; keypoints[cam][fr][i].y = xy[2 * i + 1]; }
            std::vector<float> c(3 * (size_t)m);
            if (!rd(f, c.data(), c.size())) return 2;
            kp_with_depth[cam][fr].reset(new standin::PointCloud);
            for (int j = 0; j < m; j++) kp_with_depth[cam][fr]->push_back(standin::PointXYZ(c[3 * j], c[3 * j + 1], c[3 * j + 2]));
        }
    fclose(f);
    velo_ctx* ctx = 0;
    if (velo_create(&ctx, 0) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 3; }
    velo_hip::LandmarkStore store(ctx, num_cams, &cam_trans[0]);
    standin::PointCloud::Ptr landmarks(new standin::PointCloud);
    std::vector<bool> keypoint_added;
    for (int fr = 0; fr < F; fr++) store.setPose(fr, &ceres_poses_vec[fr][0]);
    for (int fr = 0; fr < F; fr++) {
        if (store.observeFrame(fr, keypoints, keypoint_ids, has_depth, kp_with_depth) != VELO_OK ||
            store.triangulateFrame(fr, landmarks, keypoint_added) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
    }
    std::vector<int> window(F);
    for (int fr = 0; fr < F; fr++) window[fr] = fr;
    velo_ba_summary s;
    if (store.bundleAdjust(window, n_fixed, ceres_poses_vec, landmarks, &s) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 5; }
    printf("s %d %d %d %d %d %d %d %016llx %016llx\n", s.termination, s.iterations, s.evaluations, s.n_landmarks, s.n_blocks, s.n_residuals, s.n_trace,
           bits(s.initial_cost), bits(s.final_cost));
    for (int k = 0; k < s.n_trace; k++) printf("t %d %d %016llx %016llx\n", s.trace[k].iteration, s.trace[k].status, bits(s.trace[k].cost), bits(s.trace[k].candidate_cost));
    for (int fr = 0; fr < F; fr++) {
        printf("p %d", fr);
        for (int j = 0; j < 6; j++) printf(" %016llx", bits(ceres_poses_vec[fr][j]));
        printf("\n");
    }
    for (size_t id = 0; id < keypoint_added.size(); id++)
        if (keypoint_added[id]) printf("l %zu %08x %08x %08x\n", id, bits(landmarks->points[id].x), bits(landmarks->points[id].y), bits(landmarks->points[id].z));
    // a window the library refuses leaves the containers alone
    std::vector<int> bad(window.rbegin(), window.rend());
    const std::vector<std::vector<double> > kept(ceres_poses_vec);
    printf("refused %d kept %d\n", store.bundleAdjust(bad, n_fixed, ceres_poses_vec, landmarks) == VELO_ERR_INVALID ? 1 : 0, kept == ceres_poses_vec ? 1 : 0);
    velo_destroy(ctx);
    return 0;
}
