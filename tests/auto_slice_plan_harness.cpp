// Host-only harness of tests/test_auto_slice_plan_cpu.py: sweeps the engine's launch plans over frame shapes, disparity
// counts, batch limits, stream-lane modes and CU counts, and checks that every slice record a launch would write fits the
// per-lane region of the slice buffer smx_create allocates (k_match_auto.h: slice_region_floats).  The region and the
// engine's choice of the one-launch AUTO kernel come from the engine's own planner (smx_plan.h: derive_facts, plan_range);
// the HIP runtime is never called.
//
// Output: a line per violation ("overflow <kind> h w Dd B n on_lanes cus nsplit th need region": the first 50, and every
// one at the pooled shapes of the GPU tests for an MI355X (256 CUs) with max_batch = 64), then a summary line
// "checked <configs> accepted <one-launch calls> split <split exact launches> violations <count>".
#include <cstdio>
#include <vector>

#include "smx_plan.h"

using namespace smx;

static std::vector<int> with_edges(std::vector<int> v, int hi) {
    // the values either side of every band and tile edge of the plans (band rows 8 / 10 / 12 / 24, exact-order tiles
    // 16 x 128, fast windows 42 and 168 columns)
    for (int e : {8, 10, 12, 16, 24, 42, 128, 168})
        for (int d = -1; d <= 1; ++d) v.push_back(e + d);
    std::vector<int> out;
    for (int x : v)
        if (x >= 1 && x <= hi) {
            bool seen = false;
            for (int y : out) seen = seen || y == x;
            if (!seen) out.push_back(x);
        }
    return out;
}

// pooled h, w, Dd of the frames tests/test_auto_one_launch_gpu.py runs: 128x256 K=2 D=64, 64x128 K=1 D=32,
// 96x160 K=2 D=32, C2 (1242x375 K=2 D=128)
static bool gpu_test_shape(int h, int w, int Dd, int B, int cus) {
    if (B != 64 || cus != 256) return false;
    return (h == 64 && w == 128 && Dd == 32) || (h == 48 && w == 80 && Dd == 16) || (h == 187 && w == 621 && Dd == 64);
}

int main() {
    // pooled sizes up to config C4's 540 x 960; among them the shapes of the frames the GPU tests run
    // (64 x 128, 48 x 80, 187 x 621)
    const std::vector<int> hs = with_edges({1, 2, 3, 5, 20, 32, 40, 48, 64, 80, 96, 120, 160, 187, 200, 256, 300, 384, 450, 540}, 540);
    const std::vector<int> ws = with_edges({1, 2, 3, 5, 30, 48, 64, 80, 96, 160, 200, 256, 300, 336, 400, 512, 621, 700, 800, 960}, 960);
    const std::vector<int> dds = {1, 2, 3, 4, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 96, 128, 129,
                                  192, 193, 194, 256, 257, 384, 512, 640, 780, 800};
    const int bs[] = {1, 2, 4, 8, 16, 17, 32, 64, 128};
    const int cuss[] = {1, 80, 256, 304};
    long configs = 0, accepted = 0, split = 0, violations = 0;
    smx_config cfg{};
    cfg.downscale_factor = 2; cfg.ncc_patch_radius = 1; cfg.sad_patch_radius = 5; cfg.threshold = 5;
    cfg.small_mbm_radius = 1; cfg.mid_mbm_radius = 4; cfg.large_mbm_radius = 10; cfg.match_mode = SMX_MATCH_AUTO;
    CallFacts gray;
    gray.in_mode = IN_GRAY_F32;
    gray.route.grid_hint = 0;
    for (int cus : cuss)
        for (int h : hs)
            for (int w : ws)
                for (int Dd : dds)
                    for (int B : bs) {
                        // an AUTO engine of the default configuration at this pooled shape: the region of one lane
                        smx_dims d{};
                        d.K = 2; d.H = 2 * h; d.W = 2 * w; d.h = h; d.w = w; d.dmin = 0; d.dmax = Dd - 1; d.Dd = Dd;
                        cfg.max_batch = B;
                        const EngineFacts f = derive_facts(cfg, d, cus, PlanOptions{});
                        const size_t region = f.slices_floats;
                        const int tiles = f.e2_tiles;
                        MatchParams p{};
                        p.h = h; p.w = w; p.Dd = Dd;
                        const size_t hw = (size_t)h * w;
                        ++configs;
                        for (int on_lanes = 0; on_lanes < 2; ++on_lanes)
                            for (int n = 1; n <= B; ++n) {
                                // a whole f32 gray call after an on-grid report: the one call that can take the one-launch kernel
                                gray.on_lanes = on_lanes != 0;
                                const RangePlan plan = plan_range(f, gray, n, true);
                                const FastPlan &pl = plan.fast;
                                if (plan.route == AGG_AUTO_ONE_LAUNCH) {
                                    ++accepted;
                                    // auto_launch (smx_plan.h): nsplit slices, records at [sp][word][n][h][w]
                                    const int ns = match_auto_nsplit(p, pl.th);
                                    const size_t need = (size_t)ns * SMX_SLICE_WORDS * n * hw;
                                    if (need > region) {
                                        if (++violations <= 50 || gpu_test_shape(h, w, Dd, B, cus))
                                            printf("overflow auto %d %d %d %d %d %d %d %d %d %zu %zu\n", h, w, Dd, B, n, on_lanes, cus, ns,
                                                   pl.th, need, region);
                                    }
                                }
                                // exact_launch (smx_plan.h) with the split allowed: records at [sp][word][n][h][w]
                                const int sp = exact_split(tiles, n, Dd, cus);
                                if (sp > 1 && on_lanes == 0) {
                                    ++split;
                                    const size_t need = (size_t)sp * SMX_SLICE_WORDS * n * hw;
                                    if (need > region) {
                                        if (++violations <= 50 || gpu_test_shape(h, w, Dd, B, cus))
                                            printf("overflow exact %d %d %d %d %d %d %d %d %d %zu %zu\n", h, w, Dd, B, n, on_lanes, cus, sp, 0,
                                                   need, region);
                                    }
                                }
                            }
                    }
    printf("checked %ld accepted %ld split %ld violations %ld\n", configs, accepted, split, violations);
    return violations == 0 ? 0 : 1;
}
