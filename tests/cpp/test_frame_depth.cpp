// Driver of FrameStore::putFrameWithDepth / putFramesWithDepth (include/velo_frame_store.hpp) against stand-in container types: reads
// a scan and three frames of keypoints, ids and descriptor rows, and leaves them in the frame store and the landmark store of
//   context A  with putFrameWithDepth(observe),
//   context B  with today's members: velo_project_lidar + velo_depth_association per camera into has_depth / keypoints_with_depth
//              containers, then putFrame + putDescriptors + LandmarkStore::observeFrame,
//   contexts C and D  with one putFramesWithDepth call per frame,
// and prints whether A, C and D hold what B holds: every entry (velo_frames_get), the numbers of velo_frames_info /
// velo_frames_desc_info / velo_landmarks_info and velo_landmarks_get of every id.  Without an argument it only has to compile and link.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mat_standin.hpp"
#include "standins.hpp"
#include "velo_frame_store.hpp"
#include "velo_landmarks.hpp"

namespace {

typedef std::vector<std::vector<std::vector<standin::Point2f> > > Keypoints;
typedef std::vector<std::vector<std::vector<int> > > Ints;
typedef std::vector<std::vector<standin::PointCloud::Ptr> > Clouds;
typedef std::vector<std::vector<standin::Mat> > Descriptors;

template <class T>
bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

bool read_rings(FILE* f, std::vector<standin::PointCloud::Ptr>* rings) {
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

// everything the two stores of a context say, as bytes
bool state_of(velo_ctx* ctx, int num_cams, int n_frames, int max_id, std::vector<unsigned char>* out) {
    out->clear();
    const auto add = [out](const void* p, size_t bytes) { const unsigned char* b = (const unsigned char*)p; out->insert(out->end(), b, b + bytes); };
    for (int fr = 0; fr < n_frames; fr++)
        for (int cam = 0; cam < num_cams; cam++) {
            int32_t n = 0, m = 0, hr = 0;
            if (velo_frames_get(ctx, fr, cam, 0, 0, 0, 0, 0, 0, 0, &n, &m, &hr) != VELO_OK) return false;
            std::vector<int32_t> ids((size_t)n + 1), hd((size_t)n + 1);
            std::vector<float> xy(2 * (size_t)n + 2), cloud(3 * (size_t)m + 3);
            std::vector<uint8_t> rows(64 * (size_t)n + 64);
            if (velo_frames_get(ctx, fr, cam, &ids[0], &xy[0], &hd[0], &cloud[0], &rows[0], n, m, &n, &m, &hr) != VELO_OK) return false;
            add(&n, 4); add(&m, 4); add(&hr, 4);
            add(&ids[0], 4 * (size_t)n); add(&hd[0], 4 * (size_t)n); add(&xy[0], 8 * (size_t)n); add(&cloud[0], 12 * (size_t)m);
            if (hr) add(&rows[0], 64 * (size_t)n);
        }
    int32_t info[8], dinfo[4], linfo[8];
    if (velo_frames_info(ctx, info) != VELO_OK || velo_frames_desc_info(ctx, dinfo) != VELO_OK || velo_landmarks_info(ctx, linfo) != VELO_OK) return false;
    add(info, sizeof(info)); add(dinfo, sizeof(dinfo)); add(linfo, sizeof(linfo));
    std::vector<int32_t> ids((size_t)max_id + 1), cnt((size_t)max_id + 1);
    std::vector<float> xyz(3 * ((size_t)max_id + 1));
    std::vector<uint8_t> added((size_t)max_id + 1);
    for (int i = 0; i <= max_id; i++) ids[(size_t)i] = i;
    if (velo_landmarks_get(ctx, &ids[0], max_id + 1, &xyz[0], &added[0], &cnt[0]) != VELO_OK) return false;
    add(&xyz[0], 4 * xyz.size()); add(&added[0], added.size()); add(&cnt[0], 4 * cnt.size());
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { printf("frame depth adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<standin::PointCloud::Ptr> scan;
    if (!read_rings(f, &scan)) return 2;
    int num_cams = 0, n_frames = 0;
    double thresh = 0.0;
    if (!rd(f, &num_cams, 1) || !rd(f, &n_frames, 1) || !rd(f, &thresh, 1)) return 2;
    std::vector<float> cam_trans(3 * (size_t)num_cams);
    std::vector<double> bounds(4 * (size_t)num_cams);
    if (!rd(f, cam_trans.data(), cam_trans.size()) || !rd(f, bounds.data(), bounds.size())) return 2;
    Keypoints keypoints(num_cams, std::vector<std::vector<standin::Point2f> >(n_frames));
    Ints keypoint_ids(num_cams, std::vector<std::vector<int> >(n_frames)), has_depth = keypoint_ids;
    Clouds kp_with_depth(num_cams, std::vector<standin::PointCloud::Ptr>(n_frames));
    Descriptors descriptors(num_cams, std::vector<standin::Mat>(n_frames));
    int max_id = 0;
    for (int fr = 0; fr < n_frames; fr++)
        for (int cam = 0; cam < num_cams; cam++) {
            int n = 0;
            if (!rd(f, &n, 1)) return 2;
            std::vector<float> xy(2 * (size_t)n);
            keypoint_ids[cam][fr].resize(n); keypoints[cam][fr].resize(n);
            if (!rd(f, keypoint_ids[cam][fr].data(), n) || !rd(f, xy.data(), xy.size())) return 2;
            for (int i = 0; i < n; i++) {
                keypoints[cam][fr][i].x = xy[2 * i]; keypoints[cam][fr][i].y = xy[2 * i + 1];
                if (keypoint_ids[cam][fr][i] > max_id) max_id = keypoint_ids[cam][fr][i];
            }
            descriptors[cam][fr] = standin::Mat(n, 64, 80);              // rows 80 bytes apart: a ROI-like stride
            for (int i = 0; i < n; i++)
                if (!rd(f, descriptors[cam][fr].ptr<unsigned char>(i), 64)) return 2;
        }
    fclose(f);

    velo_hip::Context A(0), B(0), C(0), D(0);
    velo_hip::Context* all[4] = {&A, &B, &C, &D};
    std::vector<velo_hip::FrameStore> frames;
    std::vector<velo_hip::LandmarkStore> landmarks;
    for (int k = 0; k < 4; k++) {
        all[k]->set_source(scan);
        frames.push_back(velo_hip::FrameStore(all[k]->get(), num_cams, &cam_trans[0], 4096));
        landmarks.push_back(velo_hip::LandmarkStore(all[k]->get(), num_cams, &cam_trans[0], 128));
        if (frames.back().status() != VELO_OK || landmarks.back().status() != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 5; }
    }
    for (int fr = 0; fr < n_frames; fr++) {
        std::vector<int32_t> n_wd;
        if (frames[0].putFrameWithDepth(fr, keypoints, keypoint_ids, &descriptors, &bounds[0], thresh, true, false, &n_wd) != VELO_OK) {
            fprintf(stderr, "%s\n", velo_last_error());
            return 6;
        }
        // context B: the depth comes to the host and goes back three times
        for (int cam = 0; cam < num_cams; cam++) {
            const int n = (int)keypoints[cam][fr].size();
            std::vector<float> xy(2 * (size_t)n + 2), cloud(3 * (size_t)n + 3);
            for (int i = 0; i < n; i++) { xy[2 * i] = keypoints[cam][fr][i].x; xy[2 * i + 1] = keypoints[cam][fr][i].y; }
            has_depth[cam][fr].assign((size_t)n, -1);
            int32_t m = 0;
            std::vector<int32_t> hd((size_t)n + 1);
            if (velo_project_lidar(B.get(), 0, &cam_trans[3 * cam], &bounds[4 * cam], 0) != VELO_OK ||
                velo_depth_association(B.get(), n ? &xy[0] : 0, n, thresh, &cloud[0], n, n ? &hd[0] : 0, &m) != VELO_OK) {
                fprintf(stderr, "%s\n", velo_last_error());
                return 7;
            }
            kp_with_depth[cam][fr].reset(new standin::PointCloud);
            for (int i = 0; i < n; i++) has_depth[cam][fr][i] = hd[(size_t)i];
            for (int j = 0; j < m; j++) kp_with_depth[cam][fr]->push_back(standin::PointXYZ(cloud[3 * j], cloud[3 * j + 1], cloud[3 * j + 2]));
            if (n_wd[(size_t)cam] != m) { fprintf(stderr, "camera %d: %d depth points, the yardstick %d\n", cam, n_wd[(size_t)cam], m); return 8; }
        }
        if (frames[1].putFrame(keypoints, keypoint_ids, has_depth, kp_with_depth, fr) != VELO_OK || frames[1].putDescriptors(descriptors, fr) != VELO_OK ||
            landmarks[1].observeFrame(fr, keypoints, keypoint_ids, has_depth, kp_with_depth) != VELO_OK) {
            fprintf(stderr, "%s\n", velo_last_error());
            return 9;
        }
        velo_hip::FrameStore* two[2] = {&frames[2], &frames[3]};
        const int fr2[2] = {fr, fr};
        const Keypoints* kp2[2] = {&keypoints, &keypoints};
        const Ints* id2[2] = {&keypoint_ids, &keypoint_ids};
        const Descriptors* de2[2] = {&descriptors, &descriptors};
        const double* bo2[2] = {&bounds[0], &bounds[0]};
        if (velo_hip::FrameStore::putFramesWithDepth(two, 2, fr2, kp2, id2, de2, bo2, thresh, true) != VELO_OK) {
            fprintf(stderr, "%s\n", velo_last_error());
            return 10;
        }
    }
    std::vector<unsigned char> s[4];
    for (int k = 0; k < 4; k++)
        if (!state_of(all[k]->get(), num_cams, n_frames, max_id, &s[k])) { fprintf(stderr, "%s\n", velo_last_error()); return 11; }
    size_t with = 0, all_kp = 0;
    for (int cam = 0; cam < num_cams; cam++)
        for (int fr = 0; fr < n_frames; fr++) { with += kp_with_depth[cam][fr]->size(); all_kp += keypoints[cam][fr].size(); }
    printf("keypoints %zu with depth %zu\n", all_kp, with);
    printf("putFrameWithDepth equals putFrame + putDescriptors + observeFrame: %d\n", s[0] == s[1] ? 1 : 0);
    printf("putFramesWithDepth equals it on both contexts: %d %d\n", s[2] == s[1] ? 1 : 0, s[3] == s[1] ? 1 : 0);
    return 0;
}
