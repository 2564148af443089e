// Driver of velo_hip::ScanMap (include/velo_scan_map.hpp): reads the frames of a short drive and walks them twice as a scan-to-map
// odometry loop with a sliding window -- every frame is registered against the loaded map with the constant-velocity guess and then
// inserted with its solved pose -- once through the wrapper, once through the C-ABI calls, and prints whether poses, loaded clouds,
// windows and stored scans are the same.  Without an argument it only has to compile and link.
#include <cstdio>
#include <cstring>
#include <vector>

#include "velo_scan_map.hpp"

namespace {

struct Scan { std::vector<int32_t> off; std::vector<float> xyz; };

template <class T>
bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

void mul(const double* a, const double* b, double* c) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) c[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) + a[4 * i + 3] * b[12 + j];
}

void rigid_inverse(const double* p, double* q) {
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) q[4 * i + j] = p[4 * j + i];
        q[4 * i + 3] = -((p[i] * p[3] + p[4 + i] * p[7]) + p[8 + i] * p[11]);
    }
    q[12] = q[13] = q[14] = 0.0; q[15] = 1.0;
}

struct Walk {
    std::vector<double> poses;                  // 16 per frame
    std::vector<std::vector<float> > clouds;    // the loaded target of every registration
    std::vector<int> window;                    // the frames left at the end
    std::vector<float> last_scan;               // the newest stored scan, read back
    int evicted;
};

bool target_cloud(velo_ctx* c, std::vector<float>* out) {
    int32_t n = 0;
    if (velo_get_cloud(c, 1, 0, 0, &n) != VELO_OK) return false;
    out->assign(3 * (size_t)n + 3, 0.0f);
    return velo_get_cloud(c, 1, &(*out)[0], n, &n) == VELO_OK;
}

// the loop; map calls go through the wrapper (w) or through the C-ABI on the raw handle (m)
bool walk(velo_ctx* c, const std::vector<Scan>& scans, const double x0[6], velo_hip::ScanMap* w, velo_map* m, Walk* W) {
    const int n = (int)scans.size();
    double x[6], eye[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(x, x0, sizeof(x));
    W->poses.assign(16 * (size_t)n, 0.0);
    W->clouds.clear();
    W->evicted = 0;
    for (int k = 0; k < n; k++) {
        const Scan& s = scans[k];
        if (velo_set_source(c, &s.xyz[0], 12, &s.off[0], (int32_t)s.off.size() - 1, 0) != VELO_OK) return false;
        double* pose = &W->poses[16 * (size_t)k];
        if (k == 0) std::memcpy(pose, eye, sizeof(eye));
        else {
            double inv[16], T[16];
            rigid_inverse(pose - 16, inv);
            if ((w ? w->load(c, inv) : velo_map_load(m, c, inv)) != VELO_OK) return false;
            W->clouds.push_back(std::vector<float>());
            if (!target_cloud(c, &W->clouds.back())) return false;
            if (velo_frame_to_frame(c, x, T, 0) != VELO_OK) return false;       // x stays: the constant-velocity guess of the next frame
            mul(pose - 16, T, pose);
        }
        int gone = 0;
        if (w) { if (w->insert(c, false, k, pose, &gone) != VELO_OK) return false; }
        else { int32_t g = 0; if (velo_map_insert(m, c, 0, k, pose, &g) != VELO_OK) return false; gone = g; }
        W->evicted += gone;
    }
    if (w) {
        W->window = w->frames();
        double p[16];
        if (w->get_scan(n - 1, &W->last_scan, 0, p) != VELO_OK || std::memcmp(p, &W->poses[16 * (size_t)(n - 1)], sizeof(p)) != 0) return false;
    } else {
        int32_t f[64], np = 0;
        const int cnt = velo_map_frames(m, f, 64);
        W->window.assign(f, f + cnt);
        if (velo_map_get_scan(m, n - 1, 0, 0, &np, 0, 0, 0, 0) != VELO_OK) return false;
        W->last_scan.assign(3 * (size_t)np + 3, 0.0f);
        if (velo_map_get_scan(m, n - 1, &W->last_scan[0], np, &np, 0, 0, 0, 0) != VELO_OK) return false;
        W->last_scan.resize(3 * (size_t)np);
    }
    return true;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(&a[0], &b[0], sizeof(T) * a.size()) == 0);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        velo_hip::ScanMap* none = 0;
        (void)none;
        printf("scan map wrapper linked\n");
        return 0;
    }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_frames = 0, skip = 0, window = 0;
    double x0[6];
    if (!rd(f, &n_frames, 1) || !rd(f, &skip, 1) || !rd(f, &window, 1) || !rd(f, x0, 6)) return 2;
    std::vector<Scan> scans((size_t)n_frames);
    for (int k = 0; k < n_frames; k++) {
        int nr = 0;
        if (!rd(f, &nr, 1)) return 2;
        scans[k].off.resize((size_t)nr + 1);
        if (!rd(f, &scans[k].off[0], scans[k].off.size())) return 2;
        scans[k].xyz.resize(3 * (size_t)scans[k].off[nr]);
        if (!rd(f, &scans[k].xyz[0], scans[k].xyz.size())) return 2;
    }
    fclose(f);

    velo_ctx *a = 0, *b = 0;
    if (velo_create(&a, 0) != VELO_OK || velo_create(&b, 0) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 3; }
    velo_params P;
    velo_get_params(a, &P);
    P.icp_skip = skip;
    velo_set_params(a, &P);
    velo_set_params(b, &P);
    Walk WA, WB;
    bool ok_a = false, ok_b = false;
    {
        velo_hip::ScanMap map(0, window, 1 << 22);
        if (map.status() != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        ok_a = walk(a, scans, x0, &map, 0, &WA);
        if (!ok_a) fprintf(stderr, "wrapper walk: %s\n", velo_last_error());
        velo_hip::ScanMap::Info I;
        if (map.info(&I) != VELO_OK) return 4;
        printf("window %d scans %lld evicted %lld\n", window, (long long)I.scans, (long long)I.evictions);
        // the wrapper's batch entry with one pair is the single load
        std::vector<velo_hip::ScanMap*> ms(1, &map);
        std::vector<velo_ctx*> cs(1, a);
        std::vector<double> inv(16, 0.0);
        rigid_inverse(&WA.poses[16 * (size_t)(n_frames - 1)], &inv[0]);
        std::vector<float> one, two;
        const bool l1 = map.load(a, &inv[0]) == VELO_OK && target_cloud(a, &one);
        const bool l2 = velo_hip::ScanMap::load_batch(ms, cs, inv) == VELO_OK && target_cloud(a, &two);
        printf("batch of one equals load: %d\n", l1 && l2 && same(one, two) ? 1 : 0);
        const bool dropped = map.drop(n_frames - 1) == VELO_OK && map.drop(n_frames - 1) == VELO_ERR_STATE && map.clear() == VELO_OK && map.frames().empty();
        printf("drop and clear: %d\n", dropped ? 1 : 0);
    }
    velo_map* m = 0;
    if (velo_map_create(&m, 0, window, 1 << 22) != VELO_OK) return 5;
    ok_b = walk(b, scans, x0, 0, m, &WB);
    if (!ok_b) fprintf(stderr, "C-ABI walk: %s\n", velo_last_error());
    velo_map_destroy(m);
    bool clouds = WA.clouds.size() == WB.clouds.size();
    for (size_t k = 0; clouds && k < WA.clouds.size(); k++) clouds = same(WA.clouds[k], WB.clouds[k]);
    printf("walks ran: %d %d\n", ok_a ? 1 : 0, ok_b ? 1 : 0);
    printf("poses equal: %d clouds equal: %d window equal: %d stored scan equal: %d evicted equal: %d\n", same(WA.poses, WB.poses) ? 1 : 0, clouds ? 1 : 0,
           same(WA.window, WB.window) ? 1 : 0, same(WA.last_scan, WB.last_scan) ? 1 : 0, WA.evicted == WB.evicted ? 1 : 0);
    const double* last = &WA.poses[16 * (size_t)(n_frames - 1)];
    printf("last pose translation %.17g %.17g %.17g\n", last[3], last[7], last[11]);
    velo_destroy(a);
    velo_destroy(b);
    return 0;
}
