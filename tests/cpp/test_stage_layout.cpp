// StageLayout (csrc/velo_stage_layout.h) on its own, under the address and undefined-behaviour sanitizers: every part of every layout
// is written through in(base) into a heap block of exactly `bytes` bytes (the address sanitizer is the check that nothing leaves it),
// and the offsets are compared with the sums the launch sets spelled out by hand before the layout existed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "velo_stage_layout.h"

using velo::StageLayout;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

size_t aligned(size_t n) { return (n + 63) & ~(size_t)63; }            // the hand-written rounding of the launch sets

template <size_t N> struct Rec { unsigned char b[N]; };                // an element of N bytes, alignment 1

// every element of the part written, every byte of it; returns the bytes written
template <typename T>
size_t fill(const StageLayout::Part<T>& p, void* base, unsigned char v) {
    T* w = p.in(base);
    for (size_t i = 0; i < p.n; i++) std::memset(&w[i], v, sizeof(T));
    const T* r = p.in(static_cast<const void*>(base));
    CHECK(static_cast<const void*>(r) == static_cast<const void*>(w));
    return p.size();
}

// three parts of element sizes A, B, C and counts na, nb, nc, every one on the alignment `al`, in a block of exactly `bytes` bytes
template <size_t A, size_t B, size_t C>
void three_parts(size_t na, size_t nb, size_t nc, size_t al) {
    StageLayout L;
    const auto a = L.add<Rec<A>>(na, al);
    const auto b = L.add<Rec<B>>(nb, al);
    const auto c = L.add<Rec<C>>(nc, al);
    CHECK(a.off == 0 && a.n == na && a.end() == A * na);
    CHECK(b.off % al == 0 && c.off % al == 0);
    CHECK(b.off >= a.end() && b.off < a.end() + al);                   // no overlap, and no more padding than the alignment asks for
    CHECK(c.off >= b.end() && c.off < b.end() + al);
    CHECK(L.bytes == c.end());
    if (L.bytes == 0) return;
    unsigned char* block = static_cast<unsigned char*>(std::malloc(L.bytes));   // exactly `bytes`: one byte more written is a sanitizer report
    CHECK(block);
    std::memset(block, 0, L.bytes);
    size_t written = fill(a, block, 1) + fill(b, block, 2) + fill(c, block, 3);
    size_t seen[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < L.bytes; i++) { CHECK(block[i] <= 3); seen[block[i]]++; }
    CHECK(seen[1] == a.size() && seen[2] == b.size() && seen[3] == c.size());   // no part wrote into another
    CHECK(seen[0] == L.bytes - written);
    std::free(block);
}

void counts_and_alignments() {
    const size_t aligns[] = {1, 4, 16, 64};
    for (size_t al : aligns)
        for (size_t n = 0; n <= 70; n++) {                               // sizes 3, 12, 20, 24, 56 divide no 64-byte line
            three_parts<3, 12, 1>(n, n + 1, n, al);
            three_parts<20, 24, 56>(n, 70 - n, 1, al);
            three_parts<12, 3, 20>(n, 0, n + 2, al);                     // a zero-count part between two others
            three_parts<24, 1, 12>(5, 0, n, al);
        }
    // a zero-count part takes nothing and moves the cursor to its alignment only
    StageLayout L;
    const auto a = L.add<Rec<12>>(3);
    const auto z = L.add<Rec<20>>(0);
    const auto b = L.add<int>(2);
    CHECK(a.off == 0 && z.off == 64 && z.size() == 0 && z.end() == 64 && b.off == 64 && L.bytes == 72);
    StageLayout E;                                                       // nothing but empty parts: nothing to reserve
    CHECK(E.add<int>(0).off == 0 && E.add<Rec<56>>(0, 1).off == 0 && E.bytes == 0);
    StageLayout R;                                                       // align(): the cursor on a whole line, as an upload of whole lines wants it
    R.add<Rec<3>>(7);
    R.align(64);
    CHECK(R.bytes == 64);
    R.align(64);
    CHECK(R.bytes == 64);
}

// aligned(a) + aligned(b) + c: two tables on lines of their own and a tail behind them (jobs | level tables | points; units | jobs |
// points; units | items | offsets)
template <size_t A, size_t B, size_t C>
void shape_tables(size_t na, size_t nb, size_t nc) {
    StageLayout L;
    const auto a = L.add<Rec<A>>(na);
    const auto b = L.add<Rec<B>>(nb);
    const auto c = L.add<Rec<C>>(nc);
    const size_t a_bytes = aligned(A * na), b_bytes = aligned(B * nb);
    CHECK(a.off == 0);
    CHECK(b.off == a_bytes);
    CHECK(c.off == a_bytes + b_bytes);
    CHECK(L.bytes == a_bytes + b_bytes + C * nc);
}

// 8n | n | n tightly packed: next_xy | status | kept of a tracking call
void shape_track_out(size_t n) {
    StageLayout L;
    const auto xy = L.add<Rec<8>>(n);
    const auto st = L.add<unsigned char>(n, 1);
    const auto kp = L.add<unsigned char>(n, 1);
    CHECK(xy.off == 0 && st.off == 8 * n && kp.off == 8 * n + n);
    CHECK(L.bytes == 8 * n + 2 * n);
}

// cnt | 8s | 4s | s: the counts of a detection call on lines of their own, then xy, response and fresh of every slot packed
void shape_detect_out(size_t nj, size_t s) {
    StageLayout L;
    const auto cnt = L.add<int>(3 * nj);
    const auto xy = L.add<Rec<8>>(s);
    const auto resp = L.add<float>(s, 4);
    const auto fresh = L.add<unsigned char>(s, 1);
    const size_t cnt_bytes = aligned(sizeof(int) * 3 * nj);
    CHECK(cnt.off == 0 && xy.off == cnt_bytes);
    CHECK(resp.off == cnt_bytes + s * 8);
    CHECK(fresh.off == cnt_bytes + s * (8 + 4));
    CHECK(L.bytes == cnt_bytes + s * (8 + 4 + 1));
}

void parent_formulas() {
    for (size_t na = 0; na <= 9; na++)
        for (size_t nb = 0; nb <= 4; nb++)
            for (size_t nc = 0; nc <= 66; nc += 13) {
                shape_tables<40, 136, 8>(na, nb, nc);                    // sizes like a job table, level tables and points
                shape_tables<72, 16, 8>(na, nb, nc);
                shape_tables<56, 8, 4>(na, nb, nc + 1);
            }
    for (size_t n = 0; n <= 70; n++) shape_track_out(n);
    for (size_t nj = 0; nj <= 12; nj++)
        for (size_t cap = 0; cap <= 7; cap++) shape_detect_out(nj, nj * cap);
}

}  // namespace

int main() {
    counts_and_alignments();
    parent_formulas();
    std::printf("stage layout ok\n");
    return 0;
}
