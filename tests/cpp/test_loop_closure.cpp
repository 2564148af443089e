// Driver of the loop-closure call site of include/velo_frame_store.hpp against stand-in container types: reads a scan pair, two
// keypoint frames (frame 0 = frame2, frame 1 = frame1) and their descriptor matrices, gives frame2's keypoints a landmark each (three
// observations through velo_hip::LandmarkStore), then registers twice -- frameToFrame with the matches of velo_hip::matchFeatures on
// host matrices and a host landmarks_at_frame, frameToFrameLoop with the matches made from the resident rows and the landmarks on
// the device -- and prints whether pose, matches, good_matches and residual_type are the same.  Without an argument it only has to
// compile and link.
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "mat_standin.hpp"
#include "standins.hpp"
#include "velo_frame_store.hpp"
#include "velo_landmarks.hpp"
#include "velo_match_features.hpp"

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

typedef std::vector<std::vector<std::vector<standin::Point2f> > > Keypoints;
typedef std::vector<std::vector<std::vector<int> > > Ints;
typedef std::vector<std::vector<standin::PointCloud::Ptr> > Clouds;
typedef std::vector<std::vector<std::pair<int, int> > > Matches;

static bool read_rings(FILE* f, std::vector<standin::PointCloud::Ptr>* rings) {
    int nr = 0;
    if (!rd(f, &nr, 1)) return false;
    std::vector<int> off((size_t)nr + 1);
    if (!rd(f, off.data(), off.size())) return false;
    std::vector<float> xyz(3 * (size_t)off[nr]);
    if (!rd(f, xyz.data(), xyz.size())) return false;
    for (int r = 0; r < nr; r++) {
        standin::PointCloud::Ptr c(new standin::PointCloud);
        for (int j = off[r]; j < off[r + 1]; j++) c->push_back(standin::PointXYZ(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]));
        rings->push_back(c);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("loop closure adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<standin::PointCloud::Ptr> scans_M, scans_S;
    if (!read_rings(f, &scans_M) || !read_rings(f, &scans_S)) return 2;
    int num_cams = 0, skip = 0;
    double x0[6];
    if (!rd(f, &num_cams, 1) || !rd(f, &skip, 1) || !rd(f, x0, 6)) return 2;
    std::vector<float> cam_trans(3 * (size_t)num_cams);
    if (!rd(f, cam_trans.data(), cam_trans.size())) return 2;
    const int F = 2;
    Keypoints keypoints(num_cams, std::vector<std::vector<standin::Point2f> >(F));
    Ints keypoint_ids(num_cams, std::vector<std::vector<int> >(F)), has_depth(keypoint_ids);
    Clouds kp_with_depth(num_cams, std::vector<standin::PointCloud::Ptr>(F));
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
    // descriptors[cam][frame]: rows `step` bytes apart (a ROI-like stride where step > 64)
    std::vector<std::vector<standin::Mat> > descriptors(num_cams, std::vector<standin::Mat>(F));
    for (int fr = 0; fr < F; fr++)
        for (int cam = 0; cam < num_cams; cam++) {
            int n = 0, step = 0;
            if (!rd(f, &n, 1) || !rd(f, &step, 1)) return 2;
            descriptors[cam][fr] = standin::Mat(n, 64, step);
            if (!rd(f, descriptors[cam][fr].data.data(), descriptors[cam][fr].data.size())) return 2;
        }
    double match_thresh = 0;
    if (!rd(f, &match_thresh, 1)) return 2;
    fclose(f);

    velo_hip::Context host_ctx(0), dev_ctx(0);
    velo_hip::Rig rig;
    rig.num_cams = num_cams;
    rig.cam_trans.resize(num_cams);
    for (int cam = 0; cam < num_cams; cam++) for (int k = 0; k < 3; k++) rig.cam_trans[cam][k] = cam_trans[3 * cam + k];
    velo_hip::Context* both[2] = {&host_ctx, &dev_ctx};
    for (int k = 0; k < 2; k++) { velo_params P = both[k]->params(); P.icp_skip = skip; both[k]->set_params(P); }

    // landmarks: frame2's keypoints seen three times from the same pose (landmark frames 0..2), triangulated at the third
    velo_hip::LandmarkStore lms(dev_ctx.get(), num_cams, &cam_trans[0]);
    Keypoints lk(num_cams, std::vector<std::vector<standin::Point2f> >(3));
    Ints li(num_cams, std::vector<std::vector<int> >(3)), lh(li);
    Clouds lc(num_cams, std::vector<standin::PointCloud::Ptr>(3));
    for (int cam = 0; cam < num_cams; cam++)
        for (int fr = 0; fr < 3; fr++) { lk[cam][fr] = keypoints[cam][0]; li[cam][fr] = keypoint_ids[cam][0]; lh[cam][fr] = has_depth[cam][0]; lc[cam][fr] = kp_with_depth[cam][0]; }
    const double pose0[6] = {0, 0, 0, 0, 0, 0};
    standin::PointCloud::Ptr landmarks(new standin::PointCloud);
    std::vector<bool> keypoint_added;
    for (int fr = 0; fr < 3; fr++)
        if (lms.setPose(fr, pose0) != VELO_OK || lms.observeFrame(fr, lk, li, lh, lc) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
    if (lms.triangulateFrame(2, landmarks, keypoint_added) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
    standin::Matrix4d pose_inv;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) pose_inv(i, j) = i == j ? 1.0 : 0.0;
    pose_inv(0, 3) = 0.001; pose_inv(2, 3) = -0.002;

    // path A: matchFeatures and getLandmarksAtFrame results on the host, as main.cpp:359 and main.cpp:376-386 have them
    std::map<int, standin::PointXYZ> at;
    if (lms.landmarksAtFrame(pose_inv, 2, at) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 5; }
    Matches matches(num_cams), good_a(num_cams), good_b(num_cams), matches_b;
    velo_hip::DescriptorMatcher matcher(host_ctx.get(), match_thresh);
    matcher.matchFeatures(descriptors, 1, 0, matches);
    std::vector<std::vector<velo_hip::ResidualType> > rt_a(num_cams), rt_b(num_cams);
    std::vector<standin::KdTree> kd;
    double xa[6], xb[6];
    std::memcpy(xa, x0, sizeof(xa));
    std::memcpy(xb, x0, sizeof(xb));
    standin::Matrix4d Ta = velo_hip::frameToFrame<standin::Matrix4d>(host_ctx, rig, matches, keypoints, keypoint_ids, at, kp_with_depth, has_depth, scans_M, scans_S,
                                                                     kd, 1, 0, xa, good_a, rt_a, true);
    // path B: the same from the resident frames and rows
    velo_hip::FrameStore frames(dev_ctx.get(), num_cams, &cam_trans[0]);
    if (frames.putFrame(keypoints, keypoint_ids, has_depth, kp_with_depth, 0) != VELO_OK ||
        frames.putFrame(keypoints, keypoint_ids, has_depth, kp_with_depth, 1) != VELO_OK ||
        frames.putDescriptors(descriptors, 0) != VELO_OK || frames.putDescriptors(descriptors, 1) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 6; }
    standin::Matrix4d Tb = velo_hip::frameToFrameLoop<standin::Matrix4d>(dev_ctx, frames, 1, 0, &pose_inv, match_thresh, scans_M, scans_S, kd, xb, matches_b, good_b, rt_b, true);

    size_t n_matches = 0, n_good = 0;
    for (int cam = 0; cam < num_cams; cam++) { n_matches += matches[cam].size(); n_good += good_a[cam].size(); }
    const bool same = std::memcmp(xa, xb, sizeof(xa)) == 0 && std::memcmp(Ta.m, Tb.m, sizeof(Ta.m)) == 0 && matches == matches_b && good_a == good_b && rt_a == rt_b;
    printf("landmarks %zu matches %zu good %zu\n", at.size(), n_matches, n_good);
    printf("loop equals host: %d\n", same ? 1 : 0);
    return 0;
}
