// The exactness rule of the prefix-sum form of the fast kernel's box sums (k_match_fast.h: fast_prefix_exact,
// fast_prefix_form), compiled for the host like the plan harnesses: the engine's own lines, no HIP runtime.
//
//   prefix_exact_harness          directed checks; last line "prefix-exact checks <n> failures <m>"
//
// The largest prefix is PH at tile row th + 10: (th + 11) * 48,195 * K^2 units, which must stay below 2^24.
#include <cstdio>

#include "k_match_fast.h"

using namespace smx;

static int checks = 0, failures = 0;
static void expect(bool ok, const char *what) {
    ++checks;
    if (!ok) {
        ++failures;
        printf("failed %s\n", what);
    }
}

int main() {
    // the rule is the formula, at every height up to 128 and K = 1, 2, 4, 8
    for (int k : {1, 2, 4, 8})
        for (int th = 1; th <= 128; ++th)
            expect(fast_prefix_exact(th, k) == ((long long)(th + 11) * 48195 * k * k < (1LL << 24)), "fast_prefix_exact is (th + 11) * 48195 * K^2 < 2^24");
    // K = 2: the edge lies between 76 and 77 rows (87 * 192,780 = 16,771,860 < 16,777,216 < 88 * 192,780)
    expect(fast_prefix_exact(76, 2), "K = 2, 76 rows: exact");
    expect(!fast_prefix_exact(77, 2), "K = 2, 77 rows: not exact");
    for (int th : {8, 10, 12, 24, 27, 32, 48}) {
        expect(fast_prefix_exact(th, 2), "K = 2: exact at every band height in use");
        expect(fast_prefix_exact(th, 1), "K = 1: exact at every band height in use");
    }
    expect(fast_prefix_exact(76, 1) && fast_prefix_exact(128, 1), "K = 1: a quarter of the K = 2 sums");
    // K = 4: false at every band height at which the prefix form is in use
    for (int th : {12, 24, 27, 32, 48}) {
        expect(!fast_prefix_exact(th, 4), "K = 4: not exact at the band heights of the prefix form");
        expect(!fast_prefix_exact(th, 8), "K = 8: not exact at the band heights of the prefix form");
    }
    // ... and whatever the formula says, only the PK16 == 2 instantiations (K <= 2) ever take the form
    for (int th : {8, 10, 12, 24, 27, 32, 48})
        for (int pr : {256, 288, 320})
            for (int flags = 0; flags < 16; ++flags)
                for (int pk : {0, 1}) {
                    expect(!fast_prefix_form(th, pr, flags & 1, flags & 2, pk, flags & 4, flags & 8), "PK16 != 2 keeps the sliding sums");
                }
    // whoever takes the form satisfies the rule
    for (int th : {8, 10, 12, 24, 27, 32, 48})
        for (int flags = 0; flags < 16; ++flags)
            if (fast_prefix_form(th, 256, flags & 1, flags & 2, 2, flags & 4, flags & 8)) expect(fast_prefix_exact(th, 2), "prefix form implies the rule");
    // the 8- and 10-row latency shapes keep the sliding sums
    expect(!fast_prefix_form(8, 256, false, true, 2, false, false) && !fast_prefix_form(10, 256, false, true, 2, false, false) &&
           !fast_prefix_form(8, 320, true, true, 2, false, false), "8- and 10-row latency shapes: sliding sums");
    expect(fast_prefix_form(48, 256, false, false, 2, true, false), "stacked bands at K <= 2: prefix form");
    expect(fast_prefix_form(24, 256, false, false, 2, true, false) && fast_prefix_form(27, 288, false, false, 2, true, true) &&
           fast_prefix_form(32, 320, true, false, 2, false, false), "tall bands at K <= 2: prefix form");
    expect(fast_prefix_form(12, 256, false, true, 2, false, false) && fast_prefix_form(12, 320, false, true, 2, false, true), "12-row latency shape: prefix form");
    printf("prefix-exact checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
