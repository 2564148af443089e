// Drives include/velo_detect_features.hpp the way the reference's frame loop calls detectFeatures (velo.h:118-177, main.cpp:543-557),
// against the stand-in types of track_standin.hpp plus a stand-in key point and descriptor extractor.  Needs the GPU.
// Input (argv[1]): n_cams, width, height, the current image of every camera, Kinv of every camera, the first id, then per camera: n,
// n existing pixel points (frame 1).  The existing points enter frame 1 with ids -1 and zero descriptor rows of 8 bytes;
// detectFeaturesFrame appends to frame 1 of every camera, the lists are printed; then one detectFeatures call for camera 1 on a copy of
// the containers as they were ("single"), then the id counters.
// The stand-in extractor DELETES every key point with (x + 3 y) % 5 == 0 and writes, for the k-th key point that is left, the row
// (x & 255, x >> 8, y & 255, y >> 8, 0xAB, k & 255, k >> 8, 0xCD).
// Output, one list per line: <name> <n> values (floats as their 32-bit patterns, ids, descriptor bytes).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "track_standin.hpp"
#include "velo_detect_features.hpp"

using standin::Mat;
using standin::Matrix3f;
using standin::Point2f;
typedef std::vector<std::vector<std::vector<Point2f> > > Pts;
typedef std::vector<std::vector<std::vector<int> > > Ids;
typedef std::vector<std::vector<Mat> > Descs;

struct KeyPoint {
    Point2f pt;
    float size;
    KeyPoint(Point2f p, float s) : pt(p), size(s) {}
};

struct Extractor {
    void compute(const standin::Image&, std::vector<KeyPoint>& kps, Mat& out) const {
        std::vector<KeyPoint> left;
        for (size_t i = 0; i < kps.size(); i++)
            if (((int)kps[i].pt.x + 3 * (int)kps[i].pt.y) % 5 != 0) left.push_back(kps[i]);
        kps = left;
        out = Mat((int)kps.size(), 8, 0);
        for (size_t k = 0; k < kps.size(); k++) {
            const int x = (int)kps[k].pt.x, y = (int)kps[k].pt.y;
            unsigned char* r = &out.bytes[k * 8];
            r[0] = (unsigned char)(x & 255); r[1] = (unsigned char)(x >> 8); r[2] = (unsigned char)(y & 255); r[3] = (unsigned char)(y >> 8);
            r[4] = 0xAB; r[5] = (unsigned char)(k & 255); r[6] = (unsigned char)(k >> 8); r[7] = 0xCD;
        }
    }
};

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
    if (argc < 2) return 2;
    g_in = std::fopen(argv[1], "rb");
    if (!g_in) return 2;
    const int n_cams = rd_i(), w = rd_i(), h = rd_i();
    std::vector<standin::Image> imgs;
    for (int c = 0; c < n_cams; c++) {
        standin::Image im(h, w, (size_t)w + 5);
        for (int y = 0; y < h; y++) rd(im.data + (size_t)y * im.step, (size_t)w);
        imgs.push_back(im);
    }
    std::vector<Matrix3f> Kinv(n_cams);
    for (int c = 0; c < n_cams; c++) rd(Kinv[c].v, 36);
    const int first_id = rd_i();
    Pts kp(n_cams, std::vector<std::vector<Point2f> >(2)), kp_p = kp;
    Ids ids(n_cams, std::vector<std::vector<int> >(2));
    Descs desc(n_cams, std::vector<Mat>(2));
    for (int c = 0; c < n_cams; c++) {
        const int n = rd_i();
        for (int i = 0; i < n; i++) {
            Point2f p;
            rd(&p.x, 4); rd(&p.y, 4);
            kp_p[c][1].push_back(p);
            kp[c][1].push_back(velo_hip::detect_pixel2canonical(p, Kinv[c]));
            ids[c][1].push_back(-1);
        }
        desc[c][1] = Mat(n, 8, 0);
    }
    std::fclose(g_in);
    velo_ctx* ctx = NULL;
    if (velo_create(&ctx, 0) != VELO_OK) { std::fprintf(stderr, "velo_create: %s\n", velo_last_error()); return 3; }
    try {
        std::vector<const uint8_t*> planes;
        for (int c = 0; c < n_cams; c++) planes.push_back(imgs[c].data);
        if (velo_set_images(ctx, planes.data(), n_cams, w, h, (int32_t)imgs[0].step) != VELO_OK) throw std::runtime_error(velo_last_error());
        Pts kp2 = kp, kp2_p = kp_p;
        Ids ids2 = ids;
        Descs desc2 = desc;
        velo_hip::CornerDetector<Matrix3f> d(ctx, Kinv);
        Extractor ex;
        const Extractor* freak = &ex;
        int id_counter = first_id;
        d.detectFeaturesFrame<KeyPoint>(kp, kp_p, ids, desc, freak, imgs, id_counter, 1);
        for (int c = 0; c < n_cams; c++) print_lists("frame", kp[c][1], kp_p[c][1], ids[c][1], desc[c][1]);
        int id2 = first_id + 1000;
        d.detectFeatures<KeyPoint>(kp2[1], kp2_p[1], ids2[1], desc2[1], freak, imgs[1], id2, 1, 1);
        print_lists("single", kp2[1][1], kp2_p[1][1], ids2[1][1], desc2[1][1]);
        std::printf("counters 2 %d %d\n", id_counter, id2);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        velo_destroy(ctx);
        return 4;
    }
    velo_destroy(ctx);
    return 0;
}
