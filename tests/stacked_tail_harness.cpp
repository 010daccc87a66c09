// The march rule of the stacked bands' second pass (k_match_fast.h: fast_tail_leftover, fast_tail_leftover_rows,
// fast_tail_rows, fast_tail_rows_halves), compiled for the host like the plan harnesses: the header's own __host__ __device__
// functions, no HIP runtime.  tests/test_stacked_tail_cpu.py compares every line with the restatement in
// tests/stacked_tail_ref.py, so that the model of the tail and the kernel share one rule.
//
//   stacked_tail_harness     "left <both> <upper> <lower> <code> <rows>"        the eight leftover cases at TU = FA_TH
//                            "rows <nb> <nu> <nl> <joint> <halves>"             0 <= nb, nu, nl <= 8
//                            "lds <Dd> <bytes> <fits twice>"                    the stacked tile's LDS
//                            "xch <th> <rows>"                                  exchange rows per wave at band height th
#include <cstdio>

#include "smx_plan.h"

using namespace smx;

static_assert(fast_tail_leftover(true, true, true) == FT_HALVES && fast_tail_leftover(false, false, false) == FT_NONE, "constexpr rule");
static_assert(fast_tables(FA_STACK_TH) == 2 && fast_tables(32) == 1 && fast_tables(FA_TH) == 1, "two tables per wave in the stacked form only");

int main() {
    for (int b = 0; b < 2; ++b)
        for (int u = 0; u < 2; ++u)
            for (int l = 0; l < 2; ++l) {
                const int code = fast_tail_leftover(b, u, l);
                printf("left %d %d %d %d %d\n", b, u, l, code, fast_tail_leftover_rows(code, FA_TH));
            }
    for (int nb = 0; nb <= 8; ++nb)
        for (int nu = 0; nu <= 8; ++nu)
            for (int nl = 0; nl <= 8; ++nl)
                printf("rows %d %d %d %ld %ld\n", nb, nu, nl, fast_tail_rows(nb, nu, nl, FA_TH), fast_tail_rows_halves(nb, nu, nl, FA_TH));
    for (int th : {FA_STACK_TH, 32, 27, FA_TH, FA_TH_SMALL_TALL, FA_TH_SMALL}) printf("xch %d %d\n", th, fast_xch_rows(th));
    for (int Dd : {2, 33, 64, 67})
        printf("lds %d %zu %d\n", Dd, fast_lds_bytes<256>(FA_STACK_TH, Dd), fast_stack_fits<256>(Dd) ? 1 : 0);
    return 0;
}
