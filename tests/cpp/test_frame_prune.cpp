// Driver of FrameStore::pruneFrame / keepFrame (include/velo_frame_store.hpp) against stand-in container types: reads a scan pair and
// two keypoint frames with descriptor rows (frame 0 = frame2, frame 1 = frame1), registers frame 1 against frame 0 from the resident
// frames, then prunes frame 1 twice -- with a container transcription of removeSlightlyLessTerribleFeatures (velo.h:272-327) fed with
// the registration's good_matches, and with pruneFrame -- and prints whether all six containers are the same, and whether the
// resident frame is.  keepFrame gets the same check on frame 0 with a list made here.  Without an argument it only has to compile and link.
#include <cstdio>
#include <cstring>
#include <set>
#include <vector>

#include "mat_standin.hpp"
#include "standins.hpp"
#include "velo_frame_store.hpp"

namespace {

struct Mat : standin::Mat {                         // cv::Mat::resize(rows), which the prune of the adaptor uses
    Mat() {}
    Mat(int r, int c, int s) : standin::Mat(r, c, s) {}
    void resize(size_t r) { rows = (int)r; data.resize(r * (size_t)step); }
};

typedef std::vector<std::vector<std::vector<standin::Point2f> > > Keypoints;
typedef std::vector<std::vector<std::vector<int> > > Ints;
typedef std::vector<std::vector<standin::PointCloud::Ptr> > Clouds;
typedef std::vector<std::vector<Mat> > Descriptors;
typedef std::vector<std::vector<std::pair<int, int> > > Matches;

struct Frames {
    Keypoints keypoints, keypoints_p;
    Clouds kp_with_depth;
    Ints keypoint_ids, has_depth;
    Descriptors descriptors;
};

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

// the reference's function for one camera, on these containers: the set, the walk with j and jd++, new containers copied over the old
void prune_one(Frames& F, int cam, int frame, const std::vector<int>& firsts) {
    std::set<int> good_indices;
    for (size_t k = 0; k < firsts.size(); k++) good_indices.insert(firsts[k]);
    const int m = (int)good_indices.size(), n = (int)F.keypoints[cam][frame].size();
    std::vector<standin::Point2f> tmp_keypoints(m), tmp_keypoints_p(m);
    standin::PointCloud::Ptr tmp_kp_with_depth(new standin::PointCloud);
    std::vector<int> tmp_keypoint_ids(m), tmp_has_depth(m);
    const Mat& D = F.descriptors[cam][frame];
    Mat tmp_descriptors(m, D.cols, D.step);
    int j = 0, jd = 0;
    for (int i = 0; i < n; i++) {
        if (!good_indices.count(i)) continue;
        tmp_keypoints[j] = F.keypoints[cam][frame][i];
        tmp_keypoints_p[j] = F.keypoints_p[cam][frame][i];
        tmp_keypoint_ids[j] = F.keypoint_ids[cam][frame][i];
        std::memcpy(tmp_descriptors.ptr<unsigned char>(j), D.ptr<unsigned char>(i), (size_t)D.cols);
        const int d = F.has_depth[cam][frame][i];
        if (d != -1) {
            tmp_kp_with_depth->push_back(F.kp_with_depth[cam][frame]->at(d));
            tmp_has_depth[j] = jd++;
        } else {
            tmp_has_depth[j] = -1;
        }
        j++;
    }
    F.keypoints[cam][frame] = tmp_keypoints;
    F.keypoints_p[cam][frame] = tmp_keypoints_p;
    F.kp_with_depth[cam][frame] = tmp_kp_with_depth;
    F.keypoint_ids[cam][frame] = tmp_keypoint_ids;
    F.descriptors[cam][frame] = tmp_descriptors;
    F.has_depth[cam][frame] = tmp_has_depth;
}

bool same_points(const std::vector<standin::Point2f>& a, const std::vector<standin::Point2f>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], sizeof(standin::Point2f) * a.size()) == 0);
}

bool same(const Frames& A, const Frames& B, int cam, int frame) {
    const standin::PointCloud &ca = *A.kp_with_depth[cam][frame], &cb = *B.kp_with_depth[cam][frame];
    if (ca.size() != cb.size()) return false;
    for (size_t k = 0; k < ca.size(); k++)
        if (std::memcmp(&ca.points[k], &cb.points[k], 3 * sizeof(float)) != 0) return false;
    const Mat &da = A.descriptors[cam][frame], &db = B.descriptors[cam][frame];
    if (da.rows != db.rows) return false;
    for (int r = 0; r < da.rows; r++)
        if (std::memcmp(da.ptr<unsigned char>(r), db.ptr<unsigned char>(r), 64) != 0) return false;
    return same_points(A.keypoints[cam][frame], B.keypoints[cam][frame]) && same_points(A.keypoints_p[cam][frame], B.keypoints_p[cam][frame]) &&
           A.keypoint_ids[cam][frame] == B.keypoint_ids[cam][frame] && A.has_depth[cam][frame] == B.has_depth[cam][frame];
}

// the resident entry equals the containers
bool resident_is(velo_ctx* ctx, const Frames& A, int cam, int frame) {
    const size_t n = A.keypoints[cam][frame].size(), m = A.kp_with_depth[cam][frame]->size();
    std::vector<int32_t> ids(n + 1), hd(n + 1);
    std::vector<float> xy(2 * n + 2), cloud(3 * m + 3);
    std::vector<uint8_t> rows(64 * n + 64);
    int32_t gn = -1, gm = -1, hr = -1;
    if (velo_frames_get(ctx, frame, cam, &ids[0], &xy[0], &hd[0], &cloud[0], &rows[0], (int32_t)n, (int32_t)m, &gn, &gm, &hr) != VELO_OK) return false;
    if ((size_t)gn != n || (size_t)gm != m || hr != 1) return false;
    for (size_t i = 0; i < n; i++) {
        const standin::Point2f& p = A.keypoints[cam][frame][i];
        if (ids[i] != A.keypoint_ids[cam][frame][i] || hd[i] != A.has_depth[cam][frame][i] || std::memcmp(&xy[2 * i], &p, 8) != 0) return false;
        if (std::memcmp(&rows[64 * i], A.descriptors[cam][frame].ptr<unsigned char>((int)i), 64) != 0) return false;
    }
    for (size_t k = 0; k < m; k++)
        if (std::memcmp(&cloud[3 * k], &A.kp_with_depth[cam][frame]->points[k], 12) != 0) return false;
    return true;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) { printf("frame prune adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<standin::PointCloud::Ptr> scans_M, scans_S;
    if (!read_rings(f, &scans_M) || !read_rings(f, &scans_S)) return 2;
    int num_cams = 0, skip = 0;
    double x0[6];
    if (!rd(f, &num_cams, 1) || !rd(f, &skip, 1) || !rd(f, x0, 6)) return 2;
    std::vector<float> cam_trans(3 * (size_t)num_cams);
    if (!rd(f, cam_trans.data(), cam_trans.size())) return 2;
    const int NF = 2;
    Frames A;
    A.keypoints.assign(num_cams, std::vector<std::vector<standin::Point2f> >(NF));
    A.keypoints_p = A.keypoints;
    A.keypoint_ids.assign(num_cams, std::vector<std::vector<int> >(NF));
    A.has_depth = A.keypoint_ids;
    A.kp_with_depth.assign(num_cams, std::vector<standin::PointCloud::Ptr>(NF));
    A.descriptors.assign(num_cams, std::vector<Mat>(NF));
    for (int fr = 0; fr < NF; fr++)
        for (int cam = 0; cam < num_cams; cam++) {
            int n = 0, m = 0;
            if (!rd(f, &n, 1)) return 2;
            std::vector<float> xy(2 * (size_t)n);
            A.keypoint_ids[cam][fr].resize(n); A.has_depth[cam][fr].resize(n); A.keypoints[cam][fr].resize(n); A.keypoints_p[cam][fr].resize(n);
            if (!rd(f, A.keypoint_ids[cam][fr].data(), n) || !rd(f, xy.data(), xy.size()) || !rd(f, A.has_depth[cam][fr].data(), n) || !rd(f, &m, 1)) return 2;
            for (int i = 0; i < n; i++) {
                A.keypoints[cam][fr][i].x = xy[2 * i]; A.keypoints[cam][fr][i].y = xy[2 * i + 1];
                A.keypoints_p[cam][fr][i].x = xy[2 * i] + 1.0f; A.keypoints_p[cam][fr][i].y = xy[2 * i + 1] - 1.0f;      // the pixel twin: anything distinct
            }
            std::vector<float> c(3 * (size_t)m);
            if (!rd(f, c.data(), c.size())) return 2;
            A.kp_with_depth[cam][fr].reset(new standin::PointCloud);
            for (int j = 0; j < m; j++) A.kp_with_depth[cam][fr]->push_back(standin::PointXYZ(c[3 * j], c[3 * j + 1], c[3 * j + 2]));
            A.descriptors[cam][fr] = Mat(n, 64, 80);                  // rows 80 bytes apart: a ROI-like stride
            for (int i = 0; i < n; i++)
                if (!rd(f, A.descriptors[cam][fr].ptr<unsigned char>(i), 64)) return 2;
        }
    fclose(f);

    velo_hip::Context ctx(0);
    { velo_params P = ctx.params(); P.icp_skip = skip; ctx.set_params(P); }
    velo_hip::FrameStore frames(ctx.get(), num_cams, &cam_trans[0]);
    for (int fr = 0; fr < NF; fr++)
        if (frames.putFrame(A.keypoints, A.keypoint_ids, A.has_depth, A.kp_with_depth, fr) != VELO_OK || frames.putDescriptors(A.descriptors, fr) != VELO_OK) {
            fprintf(stderr, "%s\n", velo_last_error());
            return 6;
        }
    Matches matches, good_matches;
    std::vector<std::vector<velo_hip::ResidualType> > residual_type;
    std::vector<standin::KdTree> kd;
    velo_hip::frameToFrameResident<standin::Matrix4d>(ctx, frames, 1, 0, (const standin::Matrix4d*)0, scans_M, scans_S, kd, x0, matches, good_matches, residual_type, true);

    // frame 1: the transcription on a copy, the adaptor on the original
    Frames B = A;
    for (int cam = 0; cam < num_cams; cam++) {
        B.kp_with_depth[cam][1].reset(new standin::PointCloud(*A.kp_with_depth[cam][1]));
        std::vector<int> firsts;
        for (size_t k = 0; k < good_matches[cam].size(); k++) firsts.push_back(good_matches[cam][k].first);
        prune_one(B, cam, 1, firsts);
    }
    if (frames.pruneFrame(ctx, A.keypoints, A.keypoints_p, A.kp_with_depth, A.keypoint_ids, A.descriptors, A.has_depth, 1) != VELO_OK) {
        fprintf(stderr, "%s\n", velo_last_error());
        return 7;
    }
    bool prune_same = true, prune_resident = true;
    printf("kept");
    for (int cam = 0; cam < num_cams; cam++) {
        printf(" %zu of %zu good", A.keypoints[cam][1].size(), good_matches[cam].size());
        prune_same = prune_same && same(A, B, cam, 1);
        prune_resident = prune_resident && resident_is(ctx.get(), A, cam, 1);
    }
    printf("\nprune equals reference: %d resident: %d\n", prune_same ? 1 : 0, prune_resident ? 1 : 0);
    const int again = frames.pruneFrame(ctx, A.keypoints, A.keypoints_p, A.kp_with_depth, A.keypoint_ids, A.descriptors, A.has_depth, 1);
    printf("second prune refused: %d containers kept: %d\n", again == VELO_ERR_STATE ? 1 : 0, same(A, B, 0, 1) ? 1 : 0);

    // frame 0, camera 0: a list with duplicates, unsorted
    std::vector<int> indices;
    const int n0 = (int)A.keypoints[0][0].size();
    for (int i = n0 - 1; i >= 0; i -= 2) { indices.push_back(i); if (i % 3 == 0) indices.push_back(i); }
    prune_one(B, 0, 0, indices);
    if (frames.keepFrame(0, 0, indices, A.keypoints, A.keypoints_p, A.kp_with_depth, A.keypoint_ids, A.descriptors, A.has_depth) != VELO_OK) {
        fprintf(stderr, "%s\n", velo_last_error());
        return 8;
    }
    printf("keep equals reference: %d resident: %d\n", same(A, B, 0, 0) ? 1 : 0, resident_is(ctx.get(), A, 0, 0) ? 1 : 0);
    return 0;
}
