// Host-only harness of tests/test_config_range_cpu.py and tests/test_config_range_gpu.py: what the engine's planner
// (stereo-depth_amd/csrc/smx_plan.h) derives for the configurations of tests/config_range_cases.py.  It compiles the lines
// the engine runs (derive_facts, exact_tile_lds) and never calls the HIP runtime, so the tests can assert that a case still
// reaches the code it is aimed at -- several right-tile chunks of k_match_exact, the generic float step 6, the volume
// route -- after a later change of EX_TH, EX_TW or the planner.
//
// Input (stdin), one case per line:  <id> H W K min_disparity max_disparity ncc sad threshold small mid large
// Output, one line per case:
//   "case <id> Dd <n> exact_nd <n> exact_lds <bytes> kt <n> pitch8 <n> capture <0|1> has_volume <0|1> default_radii <0|1>
//    fast_ok <0|1> refused <0|1>"
// (refused: exact_tile_lds exceeds the 64 KB of the generic exact-order kernel even at one disparity per chunk -- smx_create's
// rule), then, for every ncc_patch_radius smx_create's range check admits,
//   "boundary ncc <rn> large <rl> exact_lds <bytes> neighbour <rl + 1> neighbour_lds <bytes>"
// the largest large_mbm_radius whose tile fits and its first refused neighbour (large -1: none fits).
#include <cstdio>
#include <cstring>

#include "smx_plan.h"

using namespace smx;

static constexpr size_t LDS_LIMIT = 64 * 1024;

static smx_config config_of(int H, int W, int K, int dmin, int dmax, int rn, int sad, int thr, int rs, int rm, int rl) {
    smx_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.height = (unsigned)H; cfg.width = (unsigned)W; cfg.downscale_factor = (unsigned)K;
    cfg.min_disparity = dmin; cfg.max_disparity = dmax;
    cfg.ncc_patch_radius = (unsigned)rn; cfg.sad_patch_radius = (unsigned)sad; cfg.threshold = thr;
    cfg.small_mbm_radius = rs; cfg.mid_mbm_radius = rm; cfg.large_mbm_radius = rl;
    cfg.max_batch = 1; cfg.match_mode = SMX_MATCH_AUTO;
    return cfg;
}

// compute_dims of smx_engine.hip (reference device_buffer.cc:3-12)
static smx_dims dims_of(const smx_config &c) {
    smx_dims d;
    const int K = (int)c.downscale_factor;
    d.H = (int)c.height; d.W = (int)c.width; d.K = K;
    d.h = (d.H + K - 1) / K; d.w = (d.W + K - 1) / K;
    d.dmin = c.min_disparity / K; d.dmax = c.max_disparity / K; d.Dd = d.dmax - d.dmin + 1;
    return d;
}

int main() {
    char id[128];
    int H, W, K, dmin, dmax, rn, sad, thr, rs, rm, rl;
    while (scanf("%127s %d %d %d %d %d %d %d %d %d %d %d", id, &H, &W, &K, &dmin, &dmax, &rn, &sad, &thr, &rs, &rm, &rl) == 12) {
        const smx_config cfg = config_of(H, W, K, dmin, dmax, rn, sad, thr, rs, rm, rl);
        const smx_dims d = dims_of(cfg);
        const EngineFacts f = derive_facts(cfg, d, 256, PlanOptions{});
        int nd = 0;
        const bool refused = exact_tile_lds(cfg, d.Dd, &nd) > LDS_LIMIT;
        printf("case %s Dd %d exact_nd %d exact_lds %zu kt %d pitch8 %d capture %d has_volume %d default_radii %d fast_ok %d refused %d\n",
               id, d.Dd, f.exact_nd, f.exact_lds, f.kt, f.pitch8, f.capture ? 1 : 0, f.has_volume ? 1 : 0, f.default_radii ? 1 : 0,
               f.fast_ok ? 1 : 0, refused ? 1 : 0);
    }
    for (rn = 0; rn <= 16; ++rn) {                     // (compute_dims: ncc_patch_radius <= 16, large_mbm_radius <= 32)
        int best = -1, nd = 0;
        size_t best_lds = 0;
        for (rl = 0; rl <= 32; ++rl) {
            const smx_config cfg = config_of(64, 128, 1, 0, 63, rn, 5, 5, 0, 0, rl);
            const size_t lds = exact_tile_lds(cfg, 64, &nd);
            if (lds <= LDS_LIMIT) { best = rl; best_lds = lds; }
        }
        const smx_config next = config_of(64, 128, 1, 0, 63, rn, 5, 5, 0, 0, best + 1);
        printf("boundary ncc %d large %d exact_lds %zu neighbour %d neighbour_lds %zu\n", rn, best, best_lds, best + 1,
               exact_tile_lds(next, 64, &nd));
    }
    return 0;
}
