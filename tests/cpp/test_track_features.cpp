// Drives include/velo_track_features.hpp the way the reference's frame loop calls its functions (velo.h:28-230, main.cpp:218-245),
// against the stand-in types of track_standin.hpp.  argv[2] selects the mode:
//   "consolidate" (host only): input K (9 floats), n, n canonical points (2 floats), n ids, cols, n x cols descriptor bytes;
//                 prints the consolidated lists
//   "track" (needs the GPU): input n_cams, width, height, the previous then the current image of every camera, K and Kinv of every
//                 camera, then per camera: n, n pixel points, n ids, n x 64 descriptor bytes (frame 0).  setImages twice,
//                 trackFeaturesFrame into frame 1, the lists of frame 1 printed, consolidateFeatures per camera, printed again; then one
//                 trackFeatures call (camera 1 of frame 0 into camera 0) on fresh containers, printed; then a call with an image that was
//                 not uploaded, which must throw.
// Output, one list per line: <name> <n> values (floats as their 32-bit patterns, ids, descriptor bytes).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "track_standin.hpp"
#include "velo_track_features.hpp"

using standin::Mat;
using standin::Matrix3f;
using standin::Point2f;
typedef std::vector<std::vector<std::vector<Point2f> > > Pts;
typedef std::vector<std::vector<std::vector<int> > > Ids;
typedef std::vector<std::vector<Mat> > Descs;

static FILE* g_in = 0;
static void rd(void* p, size_t n) { if (n && std::fread(p, 1, n, g_in) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); } }
static int rd_i() { int v; rd(&v, 4); return v; }
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

static void print_lists(const std::string& name, const std::vector<Point2f>& k, const std::vector<Point2f>& p, const std::vector<int>& ids,
                        const Mat& d) {
    std::printf("%s_k %d", name.c_str(), (int)k.size());
    for (size_t i = 0; i < k.size(); i++) std::printf(" %u %u", bits(k[i].x), bits(k[i].y));
    std::printf("\n%s_p %d", name.c_str(), (int)p.size());
    for (size_t i = 0; i < p.size(); i++) std::printf(" %u %u", bits(p[i].x), bits(p[i].y));
    std::printf("\n%s_id %d", name.c_str(), (int)ids.size());
    for (size_t i = 0; i < ids.size(); i++) std::printf(" %d", ids[i]);
    std::printf("\n%s_d %d", name.c_str(), d.rows);
    for (size_t i = 0; i < d.bytes.size(); i++) std::printf(" %d", (int)d.bytes[i]);
    std::printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    g_in = std::fopen(argv[1], "rb");
    if (!g_in) return 2;
    const std::string mode = argv[2];
    if (mode == "consolidate") {
        std::vector<Matrix3f> K(1);
        rd(K[0].v, sizeof(K[0].v));
        const int n = rd_i();
        std::vector<Point2f> kp(n), kp_p(n);
        for (int i = 0; i < n; i++) { rd(&kp[i].x, 4); rd(&kp[i].y, 4); kp_p[i] = Point2f(-1.f, -1.f); }
        std::vector<int> ids(n);
        for (int i = 0; i < n; i++) ids[i] = rd_i();
        const int cols = rd_i();
        Mat d(n, cols, 0);
        rd(d.bytes.data(), d.bytes.size());
        velo_hip::FeatureTracker<Matrix3f> t(NULL, K, K);          // consolidation is host code: no context needed
        t.consolidateFeatures(kp, kp_p, ids, d, 0);
        print_lists("cons", kp, kp_p, ids, d);
        return 0;
    }
    const int n_cams = rd_i(), w = rd_i(), h = rd_i();
    std::vector<standin::Image> prev, cur;
    for (int pass = 0; pass < 2; pass++)
        for (int c = 0; c < n_cams; c++) {
            standin::Image im(h, w, (size_t)w + 3);                   // rows 3 bytes apart of padding: the stride is passed through
            for (int y = 0; y < h; y++) rd(im.data + (size_t)y * im.step, (size_t)w);
            (pass ? cur : prev).push_back(im);
        }
    std::vector<Matrix3f> K(n_cams), Kinv(n_cams);
    for (int c = 0; c < n_cams; c++) { rd(K[c].v, 36); rd(Kinv[c].v, 36); }
    Pts kp(n_cams, std::vector<std::vector<Point2f> >(2)), kp_p = kp;
    Ids ids(n_cams, std::vector<std::vector<int> >(2));
    Descs desc(n_cams, std::vector<Mat>(2));
    for (int c = 0; c < n_cams; c++) {
        const int n = rd_i();
        for (int i = 0; i < n; i++) {
            Point2f p;
            rd(&p.x, 4); rd(&p.y, 4);
            kp_p[c][0].push_back(p);
            kp[c][0].push_back(velo_hip::pixel2canonical(p, Kinv[c]));
        }
        for (int i = 0; i < n; i++) ids[c][0].push_back(rd_i());
        desc[c][0] = Mat(n, 64, 0);
        rd(desc[c][0].bytes.data(), desc[c][0].bytes.size());
    }
    std::fclose(g_in);
    velo_ctx* ctx = NULL;
    if (velo_create(&ctx, 0) != VELO_OK) { std::fprintf(stderr, "velo_create: %s\n", velo_last_error()); return 3; }
    try {
        velo_hip::FeatureTracker<Matrix3f> t(ctx, K, Kinv);
        t.setImages(prev);
        t.setImages(cur);
        t.trackFeaturesFrame(kp, kp_p, ids, desc, 1);
        for (int c = 0; c < n_cams; c++) print_lists("frame", kp[c][1], kp_p[c][1], ids[c][1], desc[c][1]);
        for (int c = 0; c < n_cams; c++) {
            t.consolidateFeatures(kp[c][1], kp_p[c][1], ids[c][1], desc[c][1], c);
            print_lists("cons", kp[c][1], kp_p[c][1], ids[c][1], desc[c][1]);
        }
        Pts kp2(n_cams, std::vector<std::vector<Point2f> >(2)), kp2_p = kp2;
        Ids ids2(n_cams, std::vector<std::vector<int> >(2));
        Descs desc2(n_cams, std::vector<Mat>(2));
        kp2[1][0] = kp[1][0]; kp2_p[1][0] = kp_p[1][0]; ids2[1][0] = ids[1][0]; desc2[1][0] = desc[1][0];
        t.trackFeatures(kp2, kp2_p, ids2, desc2, prev[1], cur[0], 1, 0, 0, 1);
        print_lists("single", kp2[0][1], kp2_p[0][1], ids2[0][1], desc2[0][1]);
        bool threw = false;
        try { t.trackFeatures(kp2, kp2_p, ids2, desc2, cur[1], cur[0], 1, 0, 0, 1); } catch (const std::runtime_error&) { threw = true; }
        std::printf("mismatch_throws 1 %d\n", threw ? 1 : 0);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        velo_destroy(ctx);
        return 4;
    }
    velo_destroy(ctx);
    return 0;
}
