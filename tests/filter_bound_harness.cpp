// Host-only harness of tests/test_filter_bound_cpu.py and tests/test_filter_route_gpu.py: prints the numbers the filtered
// exact-order route (k_match_filter.h) computes on the host, from the library's own functions, so that the tests use the
// code's error bound and launch plans instead of copies of their formulas.  It never calls the HIP runtime.
//
// Arguments: the CU counts to plan for.  Standard input: one shape per line, "name h w Dd n" (pooled rows, columns and
// disparities, pairs per call).
// Output:
//   "E <u> <filter_error_bound_units(u)>"                                      for u = 1, 4, 16, 64
//   "plan <cus> <name> <h> <w> <Dd> <n> <small at n-1> <small at n> <th> <wide> <chunks> <words>"   per CU count and shape
// where small is 0 when the engine's planner (smx_plan.h: plan_range) gives an RGB call of that many pairs the filtered
// route and 1 when the call is too small for it, th / wide are filter_plan's band height and right-tile pitch choice at n
// pairs, chunks the right-tile stagings per pass that choice needs, and words filter_cand_words(Dd).
#include <cstdio>
#include <cstdlib>

#include "k_match_filter.h"
#include "smx_plan.h"

using namespace smx;

int main(int argc, char **argv) {
    for (double u : {1.0, 4.0, 16.0, 64.0}) printf("E %.0f %.17g\n", u, filter_error_bound_units(u));
    struct Row { char name[64]; int h, w, Dd, n; };
    Row rows[512];
    int nrows = 0;
    while (nrows < 512 && scanf("%63s %d %d %d %d", rows[nrows].name, &rows[nrows].h, &rows[nrows].w, &rows[nrows].Dd, &rows[nrows].n) == 5)
        ++nrows;
    for (int a = 1; a < argc; ++a) {
        const int cus = atoi(argv[a]);
        if (cus < 1) return 2;
        for (int i = 0; i < nrows; ++i) {
            const Row &r = rows[i];
            MatchParams p{};
            p.h = r.h; p.w = r.w; p.Dd = r.Dd;
            // an engine of the default configuration at this pooled shape, an RGB call on a caller's stream, filter allowed
            smx_config cfg{};
            cfg.downscale_factor = 2; cfg.ncc_patch_radius = 1; cfg.sad_patch_radius = 5; cfg.threshold = 5;
            cfg.small_mbm_radius = 1; cfg.mid_mbm_radius = 4; cfg.large_mbm_radius = 10; cfg.match_mode = SMX_MATCH_AUTO;
            cfg.max_batch = r.n;
            smx_dims d{};
            d.K = 2; d.H = 2 * r.h; d.W = 2 * r.w; d.h = r.h; d.w = r.w; d.dmin = 0; d.dmax = r.Dd - 1; d.Dd = r.Dd;
            const EngineFacts f = derive_facts(cfg, d, cus, PlanOptions{});
            CallFacts rgb;
            rgb.in_mode = IN_RGB_U8;
            const bool small_below = r.n > 1 ? plan_range(f, rgb, r.n - 1, true).route != AGG_FILTERED : true;
            const bool small = plan_range(f, rgb, r.n, true).route != AGG_FILTERED;
            const FilterPlan pl = filter_plan(p, r.n, cus);
            const int nd = (pl.wide ? 320 : 256) - FA_WGCOLS + 1;
            printf("plan %d %s %d %d %d %d %d %d %d %d %d %d\n", cus, r.name, r.h, r.w, r.Dd, r.n, small_below ? 1 : 0, small ? 1 : 0,
                   pl.th, pl.wide ? 1 : 0, (r.Dd + nd - 1) / nd, filter_cand_words(r.Dd));
        }
    }
    return 0;
}
