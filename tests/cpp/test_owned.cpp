// The owner of the host side's runtime handles (csrc/velo_host_types.inl: template Owned) with a test handle and a counting destroy
// function, stand-alone: construction, move, move-assignment over a live handle, self-move, reset, put() over a live handle, and the
// vector operations the retired slabs and the event pools perform (growth, erase at the front, swap).  The driver
// (tests/test_cpp_owned.py) cuts the template's text out of the .inl into owned_slice.h, so this is the code the library compiles.
#include <cstdio>
#include <utility>
#include <vector>

#include "owned_slice.h"

static int destroyed = 0, live = 0;
struct Tok { int id; };
static int destroy_tok(Tok* t) { destroyed++; live--; delete t; return 0; }
static Tok* make() { live++; return new Tok{live}; }
using T = Owned<Tok*, destroy_tok>;

#define CHECK(x) do { if (!(x)) { printf("FAILED %s (line %d)\n", #x, __LINE__); return 1; } } while (0)

int main() {
    { T a; CHECK(!a && a.get() == nullptr); }
    CHECK(destroyed == 0);
    { T a(make()); CHECK(a && live == 1); T b(std::move(a)); CHECK(!a && b && live == 1); }
    CHECK(destroyed == 1 && live == 0);
    { T a(make()), b(make()); Tok* pb = b.get(); a = std::move(b); CHECK(destroyed == 2 && a.get() == pb && !b && live == 1); }
    CHECK(destroyed == 3 && live == 0);
    { T a(make()); T& r = a; a = std::move(r); CHECK(a && live == 1 && destroyed == 3); a.reset(); CHECK(!a && destroyed == 4); a.reset(); CHECK(destroyed == 4); }
    { T a(make()); *a.put() = make(); CHECK(destroyed == 5 && live == 1); }
    CHECK(destroyed == 6 && live == 0);
    {
        std::vector<T> v;
        for (int i = 0; i < 9; i++) v.emplace_back(make());
        CHECK(live == 9 && destroyed == 6);
        v.erase(v.begin());
        CHECK(live == 8 && destroyed == 7);
        std::swap(v[0], v[0]); std::swap(v[1], v[2]);
        CHECK(live == 8 && v[0] && v[1] && v[2]);
    }
    CHECK(live == 0 && destroyed == 15);
    printf("owner ok\n");
    return 0;
}
