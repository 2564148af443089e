// Drives include/velo_match_features.hpp the way the reference's loop calls its functions (velo.h:499-590, main.cpp:351-364),
// against the stand-in matrix.  Input (argv[1], binary): n_cams, n_frames, then per cam, per frame: rows, stride, rows * stride bytes;
// then per cam, per frame: n_ids, ids.  argv[2]: "ids" (host only: matchUsingId) or "match" (everything; needs the GPU).
// Output on stdout, one list per line: <name> <n> q0 t0 q1 t1 ...
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mat_standin.hpp"
#include "velo_match_features.hpp"

typedef std::vector<std::pair<int, int> > Pairs;

static void print(const char* name, const Pairs& p) {
    std::printf("%s %d", name, (int)p.size());
    for (size_t i = 0; i < p.size(); i++) std::printf(" %d %d", p[i].first, p[i].second);
    std::printf("\n");
}

static int read_i(FILE* f) { int v = 0; if (std::fread(&v, 4, 1, f) != 1) { std::fprintf(stderr, "short input\n"); std::exit(2); } return v; }

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    const int n_cams = read_i(f), n_frames = read_i(f);
    std::vector<std::vector<standin::Mat> > desc(n_cams, std::vector<standin::Mat>(n_frames));
    for (int c = 0; c < n_cams; c++)
        for (int fr = 0; fr < n_frames; fr++) {
            const int rows = read_i(f), step = read_i(f);
            desc[c][fr] = standin::Mat(rows, 64, step);
            if (rows > 0 && std::fread(desc[c][fr].data.data(), 1, desc[c][fr].data.size(), f) != desc[c][fr].data.size()) return 2;
        }
    std::vector<std::vector<std::vector<int> > > ids(n_cams, std::vector<std::vector<int> >(n_frames));
    for (int c = 0; c < n_cams; c++)
        for (int fr = 0; fr < n_frames; fr++) {
            const int n = read_i(f);
            for (int i = 0; i < n; i++) ids[c][fr].push_back(read_i(f));
        }
    std::fclose(f);

    {   // matchUsingId, both overloads (host code)
        Pairs one;
        velo_hip::matchUsingId(ids, 0, 1, 0, 1, one);
        print("id_cam01", one);
        std::vector<Pairs> per(n_cams);
        velo_hip::matchUsingId(ids, 0, 2, per);
        for (int c = 0; c < n_cams; c++) print("id_frame", per[c]);
    }
    if (std::string(argv[2]) != "match") return 0;
    velo_ctx* ctx = nullptr;
    if (velo_create(&ctx, 0) != VELO_OK) { std::fprintf(stderr, "velo_create: %s\n", velo_last_error()); return 3; }
    {
        velo_hip::DescriptorMatcher m(ctx);
        Pairs one;
        m.matchFeatures(desc, 0, 1, 0, 1, one);                  // cam 0 of frame 0 against cam 1 of frame 1
        print("mf_cam01", one);
        std::vector<Pairs> per(n_cams);
        m.matchFeatures(desc, 0, 2, per);                        // every camera, frame 0 against frame 2
        for (int c = 0; c < n_cams; c++) print("mf_frame", per[c]);
        std::vector<int> cand;
        for (int fr = 1; fr < n_frames; fr++) cand.push_back(fr);
        std::vector<std::vector<Pairs> > batch;
        m.matchFeaturesBatch(desc, 0, cand, batch);              // frame 0 against every other frame, every camera
        for (size_t k = 0; k < cand.size(); k++)
            for (int c = 0; c < n_cams; c++) print("mf_batch", batch[k][c]);
    }
    velo_destroy(ctx);
    return 0;
}
