// The trust-region controller (csrc/velo_trust_region.h) on its own: replays scripted solves from stdin the way a solver drives the
// controller and prints its state after every line; tests/test_cpp_trust_region.py writes the scripts and checks every field.
//     solve <max_num_iterations> <max_invalid> <the nine doubles of LMParams, in order>
//     start <cost> <|x|> <max |g|>
//     invalid                                                    one line per iteration: an invalid step, or
//     step <candidate cost> <model change> <|step|> <|x|> <max |g|>   the five reduced numbers of a valid one
// Doubles are read with strtod (hex floats pass exactly) and printed with %a.  Lines of a solve that has ended are skipped.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "velo_trust_region.h"

using namespace velo;

static double next_double() {
    char tok[64];
    if (std::scanf("%63s", tok) != 1) { std::fprintf(stderr, "a number is missing\n"); std::exit(2); }
    char* end = nullptr;
    const double v = std::strtod(tok, &end);
    if (end == tok || *end) { std::fprintf(stderr, "not a number: %s\n", tok); std::exit(2); }
    return v;
}

static void report(const LMParams& Q, TrustRegion* T, int status) {
    if (!T->done) tr_head(Q, T);                               // the head of the next iteration
    std::printf("%d %d %d %d %d %d %a %a %a\n", status, T->done, T->termination, T->iteration, T->evaluations, T->refresh, T->radius, T->decrease, T->cost);
}

int main() {
    LMParams Q;
    TrustRegion T;
    std::memset(&Q, 0, sizeof(Q));
    std::memset(&T, 0, sizeof(T));
    T.done = 1;
    char word[64];
    while (std::scanf("%63s", word) == 1) {
        if (!std::strcmp(word, "solve")) {
            Q.max_num_iterations = (int)next_double(); Q.max_invalid = (int)next_double();
            Q.function_tolerance = next_double(); Q.gradient_tolerance = next_double(); Q.parameter_tolerance = next_double();
            Q.initial_radius = next_double(); Q.max_radius = next_double(); Q.min_radius = next_double();
            Q.min_relative_decrease = next_double(); Q.min_diag = next_double(); Q.max_diag = next_double();
        } else if (!std::strcmp(word, "start")) {
            const double cost = next_double(), x_norm = next_double(), g = next_double();
            tr_start(Q, &T, cost, x_norm, g);
            report(Q, &T, 0);
        } else if (!std::strcmp(word, "invalid")) {
            if (!T.done) report(Q, &T, tr_invalid(Q, &T));
        } else if (!std::strcmp(word, "step")) {
            const double cost = next_double(), model_change = next_double(), step_norm = next_double(), x_norm = next_double(), g = next_double();
            if (T.done) continue;
            int status = tr_candidate(Q, &T, cost, model_change, step_norm);
            if (status == VELO_BA_ACCEPTED) status = tr_accept(Q, &T, x_norm, g);
            report(Q, &T, status);
        } else { std::fprintf(stderr, "unknown line: %s\n", word); return 2; }
    }
    // the packed upper triangle: row-major, 21 entries, and its expansion to the full block
    if (upper6(0, 0) != 0 || upper6(0, 5) != 5 || upper6(1, 1) != 6 || upper6(2, 4) != 13 || upper6(5, 5) != 20) return 3;
    double U[27], g[6], B[36];
    for (int i = 0; i < 27; i++) U[i] = (double)i;
    expand_upper6(U, g, B);
    expand_upper6(U, nullptr, nullptr);
    for (int a = 0; a < 6; a++) {
        if (g[a] != 21.0 + a) return 3;
        for (int b = a; b < 6; b++) if (B[6 * a + b] != (double)upper6(a, b) || B[6 * b + a] != B[6 * a + b]) return 3;
    }
    return 0;
}
