// Driver of tools/visual_assembly_bench.py: producing frameToFrame's visual set for one step of n contexts,
//   a  on the host, as the adaptor does it (include/velo_frame_to_frame.hpp:162-193): velo_landmarks_at_frame read back into a
//      std::map, matchUsingId with its std::map, the gather from the nested containers, velo_set_visual
//   b  velo_frames_put of the new frame + velo_build_matches, one call per context
//   c  velo_frames_put per context + ONE velo_build_matches_batch
// Inputs: 2 cameras x `per_cam` keypoints per frame, about 80 % of a frame's ids also in the previous one, about half of the ids
// added as landmarks (three observations, one triangulation, before the clock starts).  Usage: visual_assembly_bench MODE N_CTX PER_CAM REPS
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include "standins.hpp"
#include "velo_frame_store.hpp"
#include "velo_landmarks.hpp"

typedef std::vector<std::vector<std::vector<standin::Point2f> > > Keypoints;
typedef std::vector<std::vector<std::vector<int> > > Ints;
typedef std::vector<std::vector<standin::PointCloud::Ptr> > Clouds;

static unsigned long long g_seed = 88172645463325252ull;
static double rnd() { g_seed ^= g_seed << 13; g_seed ^= g_seed >> 7; g_seed ^= g_seed << 17; return (double)(g_seed >> 11) / 9007199254740992.0; }

#define OK(x) do { if ((x) != VELO_OK) { fprintf(stderr, "%s: %s\n", #x, velo_last_error()); return 3; } } while (0)

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: visual_assembly_bench a|b|c N_CTX PER_CAM REPS\n"); return 2; }
    const char mode = argv[1][0];
    const int n_ctx = atoi(argv[2]), per_cam = atoi(argv[3]), reps = atoi(argv[4]), num_cams = 2, warm = 5;
    const float cam_trans[6] = {0.f, 0.f, 0.f, -0.537f, 0.f, 0.f};
    // two frames, used alternately as (frame1, frame2): ids k and k + per_cam / 5 overlap in 80 %
    const int F = 2;
    Keypoints keypoints(num_cams, std::vector<std::vector<standin::Point2f> >(F));
    Ints keypoint_ids(num_cams, std::vector<std::vector<int> >(F)), has_depth(keypoint_ids);
    Clouds kp_with_depth(num_cams, std::vector<standin::PointCloud::Ptr>(F));
    for (int cam = 0; cam < num_cams; cam++)
        for (int fr = 0; fr < F; fr++) {
            kp_with_depth[cam][fr].reset(new standin::PointCloud);
            std::vector<int> ids(per_cam);
            for (int i = 0; i < per_cam; i++) ids[i] = i + fr * (per_cam / 5);
            for (int i = per_cam - 1; i > 0; i--) std::swap(ids[i], ids[(int)(rnd() * (i + 1))]);
            for (int i = 0; i < per_cam; i++) {
                standin::Point2f p; p.x = (float)(rnd() - 0.5); p.y = (float)(0.3 * (rnd() - 0.5));
                keypoints[cam][fr].push_back(p);
                keypoint_ids[cam][fr].push_back(ids[i]);
                if (rnd() < 0.4) {
                    has_depth[cam][fr].push_back((int)kp_with_depth[cam][fr]->size());
                    const float z = (float)(5.0 + 30.0 * rnd());
                    kp_with_depth[cam][fr]->push_back(standin::PointXYZ(p.x * z, p.y * z, z));
                } else has_depth[cam][fr].push_back(-1);
            }
        }
    std::vector<velo_ctx*> ctxs(n_ctx);
    std::vector<velo_hip::LandmarkStore*> lms(n_ctx);
    std::vector<velo_hip::FrameStore*> frs(n_ctx);
    const double pose0[6] = {0, 0, 0, 0, 0, 0};
    standin::Matrix4d pose_inv;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) pose_inv(i, j) = i == j ? 1.0 : 0.0;
    for (int c = 0; c < n_ctx; c++) {
        OK(velo_create(&ctxs[c], 0));
        // landmarks: the even ids of camera 0's frame 0, seen three times from one pose and triangulated (about half of all ids)
        lms[c] = new velo_hip::LandmarkStore(ctxs[c], num_cams, cam_trans);
        std::vector<int32_t> ids, hd;
        std::vector<float> xy;
        for (int i = 0; i < per_cam; i++)
            if (keypoint_ids[0][0][i] % 2 == 0) { ids.push_back(keypoint_ids[0][0][i]); hd.push_back(-1); xy.push_back(keypoints[0][0][i].x); xy.push_back(keypoints[0][0][i].y); }
        for (int fr = 0; fr < 3; fr++) {
            OK(lms[c]->setPose(fr, pose0));
            OK(velo_landmarks_observe(ctxs[c], fr, 0, ids.data(), xy.data(), hd.data(), 0, 0, (int32_t)ids.size()));
            OK(velo_landmarks_observe(ctxs[c], fr, 1, 0, 0, 0, 0, 0, 0));
        }
        int32_t n_tri = 0;
        OK(velo_landmarks_triangulate(ctxs[c], 2, 0, 0, 0, 0, &n_tri));
        frs[c] = new velo_hip::FrameStore(ctxs[c], num_cams, cam_trans);
        OK(frs[c]->putFrame(keypoints, keypoint_ids, has_depth, kp_with_depth, 0));
        OK(frs[c]->putFrame(keypoints, keypoint_ids, has_depth, kp_with_depth, 1));
        OK(velo_synchronize(ctxs[c]));
    }
    double M[16];
    for (int r = 0; r < 4; r++) for (int k = 0; k < 4; k++) M[4 * r + k] = pose_inv(r, k);
    std::vector<double> us;
    long long total = 0;
    for (int rep = 0; rep < warm + reps; rep++) {
        const int frame1 = rep & 1, frame2 = frame1 ^ 1;
        const auto t0 = std::chrono::steady_clock::now();
        total = 0;
        if (mode == 'a') {
            for (int c = 0; c < n_ctx; c++) {
                std::map<int, standin::PointXYZ> at;
                OK(lms[c]->landmarksAtFrame(pose_inv, 2, at));
                std::vector<velo_match> recs;
                for (int cam = 0; cam < num_cams; cam++) {
                    std::vector<std::pair<int, int> > mc;
                    std::map<int, int> id2ind;                                                    // velo.h:570-579
                    for (size_t ind = 0; ind < keypoint_ids[cam][frame1].size(); ind++) id2ind[keypoint_ids[cam][frame1][ind]] = (int)ind;
                    for (size_t ind = 0; ind < keypoint_ids[cam][frame2].size(); ind++)
                        if (id2ind.count(keypoint_ids[cam][frame2][ind])) mc.push_back(std::make_pair(id2ind[keypoint_ids[cam][frame2][ind]], (int)ind));
                    for (size_t i = 0; i < mc.size(); i++) {                                      // the adaptor's lines 166-191
                        const int point1 = mc[i].first, point2 = mc[i].second;
                        const int id = keypoint_ids[cam][frame2][point2];
                        bool d1 = has_depth[cam][frame1][point1] != -1, d2 = has_depth[cam][frame2][point2] != -1;
                        velo_match m;
                        std::memset(&m, 0, sizeof(m));
                        std::map<int, standin::PointXYZ>::const_iterator lm = at.find(id);
                        if (lm != at.end()) { m.p3_2[0] = lm->second.x; m.p3_2[1] = lm->second.y; m.p3_2[2] = lm->second.z; d2 = true; }
                        else if (d2) { const standin::PointXYZ& p = kp_with_depth[cam][frame2]->at(has_depth[cam][frame2][point2]); m.p3_2[0] = p.x; m.p3_2[1] = p.y; m.p3_2[2] = p.z; }
                        if (d1) { const standin::PointXYZ& p = kp_with_depth[cam][frame1]->at(has_depth[cam][frame1][point1]); m.p3_1[0] = p.x; m.p3_1[1] = p.y; m.p3_1[2] = p.z; }
                        m.p2_1[0] = keypoints[cam][frame1][point1].x; m.p2_1[1] = keypoints[cam][frame1][point1].y;
                        m.p2_2[0] = keypoints[cam][frame2][point2].x; m.p2_2[1] = keypoints[cam][frame2][point2].y;
                        for (int k = 0; k < 3; k++) m.t_cam[k] = cam_trans[3 * cam + k];
                        m.cam = cam; m.point1 = point1; m.point2 = point2; m.d1 = d1 ? 1 : 0; m.d2 = d2 ? 1 : 0;
                        recs.push_back(m);
                    }
                }
                OK(velo_set_visual(ctxs[c], recs.empty() ? 0 : recs.data(), (int32_t)recs.size()));
                total += (long long)recs.size();
            }
        } else {
            std::vector<int32_t> f1(n_ctx, frame1), f2(n_ctx, frame2), n_out(n_ctx, 0), per(8 * (size_t)n_ctx, 0);
            std::vector<double> Ms;
            for (int c = 0; c < n_ctx; c++) {
                OK(frs[c]->putFrame(keypoints, keypoint_ids, has_depth, kp_with_depth, frame1));   // the new frame arrives
                Ms.insert(Ms.end(), M, M + 16);
                if (mode == 'b') OK(velo_build_matches(ctxs[c], frame1, frame2, M, &per[8 * (size_t)c], 0, 0, &n_out[c]));
            }
            if (mode == 'c') OK(velo_build_matches_batch(ctxs.data(), n_ctx, f1.data(), f2.data(), Ms.data(), per.data(), 0, 0, n_out.data()));
            for (int c = 0; c < n_ctx; c++) total += n_out[c];
        }
        const double dt = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        if (rep >= warm) us.push_back(dt);
    }
    std::sort(us.begin(), us.end());
    printf("step mode=%c n_ctx=%d per_cam=%d records=%lld host_us median=%.1f min=%.1f max=%.1f reps=%d\n", mode, n_ctx, per_cam, total,
           us[us.size() / 2], us.front(), us.back(), reps);
    for (int c = 0; c < n_ctx; c++) { delete frs[c]; delete lms[c]; velo_destroy(ctxs[c]); }
    return 0;
}
