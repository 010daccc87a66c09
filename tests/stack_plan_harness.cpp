// The rule that plans the stacked bands of the throughput aggregation kernel (k_match_fast.h: match_fast_plan, FA_STACK;
// smx_plan.h: plan_range, fast_launch, match_geometry), compiled for the host like the other plan harnesses: the engine's
// own lines, no HIP runtime.  A stacked launch marches two 24-row unit bands in one go (48 output rows for 70 marched
// ones); it is planned for the sparse form on the stream lanes where that marches fewer rows, keeps th = 24 as the unit
// height and says stack = 2.
//
//   stack_plan_harness            directed checks; last line "stack-plan checks <n> failures <m>"
#include <cstdio>
#include <cstring>

#include "smx_plan.h"

using namespace smx;

static int checks = 0, failures = 0;
static void expect(bool ok, const char *what) {
    ++checks;
    if (!ok) {
        ++failures;
        printf("failed %s\n", what);
    }
}

struct Shape { int K, h, w, Dd, dmin; };
static EngineFacts facts_of(const Shape &s, int cus, PlanOptions opt) {
    smx_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.height = (unsigned)(s.h * s.K); cfg.width = (unsigned)(s.w * s.K); cfg.downscale_factor = (unsigned)s.K;
    cfg.min_disparity = s.dmin * s.K; cfg.max_disparity = (s.dmin + s.Dd) * s.K - 1;
    cfg.ncc_patch_radius = 1; cfg.sad_patch_radius = 5; cfg.threshold = 5;
    cfg.small_mbm_radius = 1; cfg.mid_mbm_radius = 4; cfg.large_mbm_radius = 10;
    cfg.max_batch = 64; cfg.match_mode = SMX_MATCH_FAST_GRID;
    smx_dims d;
    d.H = s.h * s.K; d.W = s.w * s.K; d.K = s.K; d.h = s.h; d.w = s.w; d.dmin = s.dmin; d.dmax = s.dmin + s.Dd - 1; d.Dd = s.Dd;
    return derive_facts(cfg, d, cus, opt);
}

static RangePlan plan(const EngineFacts &f, bool lanes, int n, bool dense = false) {
    CallFacts call;
    call.in_mode = IN_GRAY_U8;
    call.on_lanes = lanes;
    call.route.fast_dense = dense;
    return plan_range(f, call, n, true);
}

int main() {
    const int cus = 256;
    const Shape c2{2, 188, 621, 64, 0};                     // 375 x 1242 at K = 2, disparities 0 .. 127
    PlanOptions by_rule, never, always;
    never.fast_stack = 0;
    always.fast_stack = 1;

    {   // C2, 32 pairs (a half of the benchmark's step) on the stream lanes: 4 bands of 70 marched rows instead of 7 of 49
        const EngineFacts f = facts_of(c2, cus, by_rule);
        const RangePlan p = plan(f, true, 32);
        expect(p.route == AGG_FAST && !p.fast.small, "C2 x 32 on the lanes: throughput shape of the fast kernel");
        expect(p.fast.th == 24 && p.fast.stack == 2, "C2 x 32 on the lanes: plan th 24, stack 2");
        expect(p.fast_launch.th == 24 && p.fast_launch.stack == 2 && p.fast_launch.pitch == 256 && p.fast_launch.form == FAST_SPARSE &&
               p.fast_launch.argb && p.fast_launch.pk == 2, "C2 x 32 on the lanes: launch th 24, stack 2, pitch 256, sparse, byte-packed, pk 2");
        smx_match_geometry g;
        memset(&g, 0, sizeof(g));
        match_geometry(f, true, 32, &g);
        expect(g.band_rows == 48 && g.rows_marched == 70 && g.workgroups == 4 * 4 * 32, "geometry: 48-row bands, 70 marched rows, 4 x 4 workgroups per pair");
        // the same call ...
        const RangePlan caller = plan(f, false, 32);
        expect(!caller.fast.small && caller.fast.stack == 1 && caller.fast_launch.stack == 1 && caller.fast_launch.th == 27, "... on a caller's stream: 27-row bands");
        const RangePlan dense = plan(f, true, 32, true);
        expect(dense.dense && dense.fast.stack == 1 && dense.fast_launch.stack == 1 && dense.fast_launch.form == FAST_DENSE && dense.fast_launch.th == 27,
               "... in the dense form: 27-row bands");
        const RangePlan small = plan(f, true, 4);
        expect(small.fast.small && small.fast.stack == 1 && small.fast_launch.stack == 1, "... of 4 pairs (latency shape): not stacked");
        memset(&g, 0, sizeof(g));
        match_geometry(f, false, 32, &g);
        expect(g.band_rows == 27 && g.rows_marched == 49, "geometry on a caller's stream: 27-row bands");
    }
    {   // ... with min_disparity > 0 (the capture route: arg-max only)
        const Shape cap{2, 188, 621, 64, 8};
        const RangePlan p = plan(facts_of(cap, cus, by_rule), true, 32);
        expect(p.capture_follows && p.fast_launch.form == FAST_PASS1_ONLY && p.fast.stack == 1 && p.fast_launch.stack == 1, "pass1_only: not stacked");
    }
    {   // ... when the option forbids the form; and forced on a caller's stream
        const RangePlan p = plan(facts_of(c2, cus, never), true, 32);
        expect(p.fast.stack == 1 && p.fast_launch.stack == 1 && p.fast_launch.th == 27, "SMX_FAST_STACK=0: 27-row bands");
        const RangePlan q = plan(facts_of(c2, cus, always), false, 32);
        expect(q.fast.stack == 2 && q.fast_launch.stack == 2 && q.fast_launch.th == 24, "SMX_FAST_STACK=1 on a caller's stream: stacked");
        const RangePlan d = plan(facts_of(c2, cus, always), true, 32, true);
        expect(d.fast_launch.stack == 1 && d.fast_launch.form == FAST_DENSE, "SMX_FAST_STACK=1, dense call: no stacked dense instantiation");
        const RangePlan s = plan(facts_of(c2, cus, always), true, 4);
        expect(s.fast.small && s.fast_launch.stack == 1, "SMX_FAST_STACK=1, latency shape: not stacked");
    }
    {   // only the pitch-256 tile (up to 67 disparities) has an instantiation, in all three packed-sum forms
        const Shape wide{2, 188, 621, 96, 0}, d67{2, 188, 621, 67, 0}, d68{2, 188, 621, 68, 0}, k8{8, 188, 621, 64, 0}, k4{4, 188, 621, 64, 0};
        expect(plan(facts_of(wide, cus, always), true, 32).fast_launch.stack == 1, "96 disparities (pitch 288): not stacked");
        expect(plan(facts_of(d68, cus, always), true, 32).fast_launch.stack == 1, "68 disparities (pitch 288): not stacked");
        expect(plan(facts_of(d67, cus, by_rule), true, 32).fast_launch.stack == 2, "67 disparities (pitch 256): stacked");
        const RangePlan p8 = plan(facts_of(k8, cus, by_rule), true, 32);
        expect(p8.fast_launch.stack == 2 && p8.fast_launch.pk == 0, "K = 8: stacked, pk 0");
        const RangePlan p = plan(facts_of(k4, cus, by_rule), true, 32);
        expect(p.fast_launch.stack == 2 && p.fast_launch.pk == 1, "K = 4: stacked, pk 1");
    }
    {   // only where fewer rows are marched: h = 96 is 4 x 46 = 184 rows at 24-row bands, 2 x 70 = 140 stacked; h = 54 is
        // 2 x 49 = 98 at 27-row bands and 2 x 70 = 140 stacked
        const Shape h96{2, 96, 621, 64, 0}, h54{2, 54, 621, 64, 0};
        expect(plan(facts_of(h96, cus, by_rule), true, 64).fast_launch.stack == 2, "h = 96: stacked");
        const RangePlan p = plan(facts_of(h54, cus, by_rule), true, 64);
        expect(!p.fast.small && p.fast_launch.stack == 1 && p.fast_launch.th == 27, "h = 54: 27-row bands march fewer rows");
    }
    {   // the tile fits a CU's 160 KB twice and not three times, at the 1280-byte allocation granule, for every range of pitch 256
        for (int Dd = 1; Dd <= FA_WIDE_FROM; ++Dd) {
            const size_t granule = 1280, lds = fast_lds_bytes<256>(FA_STACK_TH, Dd), r = (lds + granule - 1) / granule * granule;
            if (Dd == 64) expect(lds == 68608 && r == 69120, "64 disparities: 68,608 bytes, 69,120 allocated");
            expect(2 * r <= 160 * 1024 && 3 * r > 160 * 1024 && fast_stack_fits<256>(Dd), "stacked tile: twice, not three times");
        }
        expect(FA_STACK_TH == 48 && FA_STACK == 2, "two 24-row unit bands");
    }
    printf("stack-plan checks %d failures %d\n", checks, failures);
    return failures != 0;
}
