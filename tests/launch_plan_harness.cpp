// Host-only harness of tests/test_launch_plan_cpu.py: the engine's launch planner (stereo-depth_amd/csrc/smx_plan.h) against
// its own prediction, its invariants and a table written by hand.  It compiles the lines the engine runs and never calls
// the HIP runtime.
//
//   1. Prediction equals execution.  call_kind() tells the content switches whether a call's default route holds a launch
//      that reports to them; the right-hand side is evaluated here from the RangePlan fields enqueue_range reads.
//   2. Plan invariants, over the sweep (configurations x match modes x entries x lanes x pairs x halves x decisions x
//      forced options x CU counts).
//   3. The directed table: the plans of today's rules for the cases a reader would ask about first.
//
// Output: a line per violation ("violation <what>: <inputs>", the first 60), then
//   "launch-plan plans <n> kinds <n> directed <n> routes <FILTERED> <EXACT> <FAST> <AUTO_ONE_LAUNCH> <AUTO_GATED> refused <n>
//    refine <FLOAT> <INT> <INT_V> <AUTO> <AUTO_V> hash <fnv-1a of every (inputs -> plan) of the sweep> violations <n>".
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "smx_plan.h"

using namespace smx;

static long violations = 0;
static void violation(const char *fmt, ...) {
    if (++violations > 60) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    printf("violation %s\n", buf);
}

struct Config {
    bool default_radii = true;
    int K = 2, h = 188, w = 621, Dd = 64, dmin = 0, sad = 5, B = 64;
    int match_mode = SMX_MATCH_AUTO, exact_filter = 0, cus = 256;
    PlanOptions opt;
};

static EngineFacts facts_of(const Config &c) {
    smx_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.height = (unsigned)(c.h * c.K); cfg.width = (unsigned)(c.w * c.K); cfg.downscale_factor = (unsigned)c.K;
    cfg.min_disparity = c.dmin * c.K; cfg.max_disparity = (c.dmin + c.Dd) * c.K - 1;
    cfg.ncc_patch_radius = 1; cfg.sad_patch_radius = (unsigned)c.sad; cfg.threshold = 5;
    cfg.small_mbm_radius = c.default_radii ? 1 : 2; cfg.mid_mbm_radius = c.default_radii ? 4 : 3; cfg.large_mbm_radius = c.default_radii ? 10 : 8;
    cfg.max_batch = c.B; cfg.match_mode = c.match_mode; cfg.exact_filter = c.exact_filter;
    smx_dims d;
    d.H = c.h * c.K; d.W = c.w * c.K; d.K = c.K; d.h = c.h; d.w = c.w; d.dmin = c.dmin; d.dmax = c.dmin + c.Dd - 1; d.Dd = c.Dd;
    return derive_facts(cfg, d, c.cus, c.opt);
}

static const char *describe(const Config &c, const CallFacts &call, int n, bool whole) {
    static char buf[256];
    snprintf(buf, sizeof(buf), "radii %d K %d %dx%d Dd %d dmin %d sad %d B %d mode %d filter %d cus %d opt %d %d | in %d lanes %d dense %d filt %d hint %d | n %d whole %d",
             c.default_radii ? 1 : 0, c.K, c.h, c.w, c.Dd, c.dmin, c.sad, c.B, c.match_mode, c.exact_filter, c.cus, c.opt.fast_dense, c.opt.fast_dense_small,
             call.in_mode, call.on_lanes ? 1 : 0, call.route.fast_dense ? 1 : 0, call.route.use_filter ? 1 : 0, call.route.grid_hint, n, whole ? 1 : 0);
    return buf;
}

// ---- the sweep -----------------------------------------------------------------------------------------------------------
static unsigned long long plan_hash = 1469598103934665603ull;
static void mix(long long v) {
    for (int i = 0; i < 8; ++i) {
        plan_hash ^= (unsigned long long)(v >> (8 * i)) & 0xffull;
        plan_hash *= 1099511628211ull;
    }
}
static long plans = 0, kinds = 0, refused = 0, routes[AGG_ROUTES] = {}, refines[5] = {};

static void check_plan(const Config &c, const EngineFacts &f, const CallFacts &call, int n, bool whole) {
    const RangePlan p = plan_range(f, call, n, whole);
    ++plans;
    const bool refuse = c.match_mode == SMX_MATCH_FAST_GRID && (!f.fast_ok || f.has_volume);
    if ((p.status != SMX_OK) != refuse || (p.status != SMX_OK && (p.status != SMX_ERR_UNSUPPORTED || !p.refusal)))
        violation("refusal: %s", describe(c, call, n, whole));
    if (p.status != SMX_OK) {
        ++refused;
        mix(p.status);
        return;
    }
    routes[p.route]++;
    refines[p.refine_kind]++;
    // every field enqueue_range reads, one per bit field (the stride as the launch gets it: only with a report)
    unsigned long long word = 0;
    for (unsigned v : {(unsigned)p.mode, (unsigned)p.route, (unsigned)p.gated_dense_first, (unsigned)p.exact_split, (unsigned)p.capture_follows,
                       (unsigned)p.fast.small, (unsigned)p.fast.th, (unsigned)p.fast.wide, (unsigned)p.dense, (unsigned)p.dense_small, (unsigned)p.reports,
                       (unsigned)(p.fill_publishes ? p.stride : 0), (unsigned)p.fill_publishes, (unsigned)p.owns_gray, (unsigned)p.refine_kind,
                       (unsigned)p.kt, (unsigned)p.refine_apron, (unsigned)p.refine_reports_grid, (unsigned)p.fill_px})
        word = word * 67 + v;
    mix((long long)word);
    const bool rgb = call.in_mode == IN_RGB_F32 || call.in_mode == IN_RGB_U8;
    if (p.route == AGG_AUTO_ONE_LAUNCH) {
        MatchParams mp{};
        mp.h = f.h; mp.w = f.w; mp.Dd = f.Dd;
        if (!f.default_radii || !p.fast.small || call.route.grid_hint != 0 || f.capture || f.has_volume || p.mode != SMX_MATCH_AUTO ||
            match_auto_slice_floats(mp, n, p.fast.th) > f.slices_floats)
            violation("one-launch: %s", describe(c, call, n, whole));
    }
    if (p.route == AGG_FILTERED && (!rgb || p.fast.small || !f.filter_ok || p.mode != SMX_MATCH_EXACT_ORDER || !call.route.use_filter))
        violation("filtered: %s", describe(c, call, n, whole));
    if (p.gated_dense_first && (p.route != AGG_FILTERED || call.in_mode != IN_RGB_F32)) violation("gated dense: %s", describe(c, call, n, whole));
    if (p.exact_split && !whole) violation("split of a half: %s", describe(c, call, n, whole));
    if (p.capture_follows != f.capture) violation("capture: %s", describe(c, call, n, whole));
    if (p.fill_publishes != (p.has_fast_launch() && !p.dense && !p.dense_small && p.reports)) violation("fill publishes: %s", describe(c, call, n, whole));
    if (p.dense && p.dense_small) violation("both dense forms: %s", describe(c, call, n, whole));
    if ((p.dense || p.dense_small) && (f.capture || f.Dd > FA_BITWORDS * 32 || !p.has_fast_launch())) violation("dense form: %s", describe(c, call, n, whole));
    if ((p.mode == SMX_MATCH_EXACT_ORDER) != (p.route == AGG_FILTERED || p.route == AGG_EXACT) || (p.mode == SMX_MATCH_FAST_GRID) != (p.route == AGG_FAST))
        violation("mode: %s", describe(c, call, n, whole));
    if (p.fill_px != (call.on_lanes && n > 4 ? 4 : 8)) violation("fill width: %s", describe(c, call, n, whole));
    if (p.refine_reports_grid && (p.refine_kind != REFINE_AUTO || !whole)) violation("grid report: %s", describe(c, call, n, whole));
}

// what an executor of the plans of a call's range(s) under the default decision would do, against call_kind
static void check_kind(const Config &c, const EngineFacts &f, int in_mode, bool on_lanes, int n0, int n1) {
    CallFacts call;
    call.in_mode = in_mode;
    call.on_lanes = on_lanes;
    call.route.fast_dense = false;
    call.route.use_filter = true;
    bool filter_reports = false, fast_reports = false;
    for (int hint = -1; hint <= 1; ++hint) {           // (the prediction does not know the hint: it must hold for each)
        call.route.grid_hint = hint;
        bool filt = false, fast = false;
        for (int n : {n0, n1}) {
            if (n < 1) continue;
            const RangePlan p = plan_range(f, call, n, n1 < 1);
            if (p.status != SMX_OK) continue;
            // enqueue_range: the sparse exact-order launch of the filtered route gets the report words; a fast launch whose
            // form is sparse gets the counter, and the fill launch publishes it
            if (p.route == AGG_FILTERED && f.filter_words) filt = true;
            if ((p.route == AGG_FAST || p.route == AGG_AUTO_ONE_LAUNCH || p.route == AGG_AUTO_GATED) && p.fill_publishes) fast = true;
        }
        if (hint == -1) { filter_reports = filt; fast_reports = fast; }
        else if (filt != filter_reports || fast != fast_reports) violation("kind depends on the hint: %s", describe(c, call, n0, n1 < 1));
    }
    const CallKind k = call_kind(f, in_mode, on_lanes, n0, n1);
    ++kinds;
    mix(k.filter_reports);
    mix(k.fast_reports);
    if (k.filter_reports != filter_reports || k.fast_reports != fast_reports) {
        call.route.grid_hint = -1;
        violation("prediction %d %d, execution %d %d (n1 %d): %s", k.filter_reports ? 1 : 0, k.fast_reports ? 1 : 0, filter_reports ? 1 : 0,
                  fast_reports ? 1 : 0, n1, describe(c, call, n0, n1 < 1));
    }
}

static void sweep_facts(const Config &c) {
    const EngineFacts f = facts_of(c);
    if (f.capture != (c.default_radii && c.dmin > 0 && c.dmin <= c.Dd) || f.has_volume != (c.dmin > 0 && !f.capture) || (f.filter_ok && f.has_volume))
        violation("facts: %s", describe(c, CallFacts{}, 0, false));
    for (int in_mode : {IN_GRAY_F32, IN_RGB_F32, IN_GRAY_U8, IN_RGB_U8})
        for (int on_lanes = 0; on_lanes < 2; ++on_lanes)
            for (int n = 1; n <= c.B; ++n) {
                check_kind(c, f, in_mode, on_lanes != 0, n, 0);
                if (on_lanes && n >= 2) check_kind(c, f, in_mode, true, (n + 1) / 2, n - (n + 1) / 2);
                CallFacts call;
                call.in_mode = in_mode;
                call.on_lanes = on_lanes != 0;
                for (int whole = 0; whole < 2; ++whole)
                    for (int dense = 0; dense < 2; ++dense)
                        for (int filt = 0; filt < 2; ++filt)
                            for (int hint = -1; hint <= 1; ++hint) {
                                call.route.fast_dense = dense != 0;
                                call.route.use_filter = filt != 0;
                                call.route.grid_hint = hint;
                                check_plan(c, f, call, n, whole != 0);
                            }
            }
}

static void sweep() {
    const int shapes[4][2] = {{48, 80}, {64, 128}, {187, 621}, {540, 960}};
    const int forced[9][2] = {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}, {-1, 1}, {0, 0}, {0, 1}, {1, 0}, {1, 1}};
    for (int radii = 0; radii < 2; ++radii)
        for (int K = 1; K <= 4; ++K)
            for (int dmin : {0, 8, 300})                       // none / capture (default radii) / aggregated volume
                for (const auto &shape : shapes)
                    for (int Dd : {16, 64, 194, 257})
                        for (int B : {1, 4, 64})
                            for (int mode : {SMX_MATCH_AUTO, SMX_MATCH_EXACT_ORDER, SMX_MATCH_FAST_GRID})
                                for (int cus : {80, 256, 304})
                                    for (int sad : {5, 4})
                                        for (const auto &opt : forced) {
                                            // Configurations that can only take the exact-order route or be refused,
                                            // whatever the shape (other radii, K = 3, the volume of default radii), at one
                                            // shape and range; the other CU counts in AUTO mode, which has every route.  On
                                            // the MI355X's 256 CUs also: the forced forms of the fast kernel, where there is
                                            // one and K does not matter to it (default radii, K = 2, not EXACT_ORDER mode),
                                            // and the other step-6 radius at one range (step 6 does not depend on it).
                                            const bool defaults = opt[0] == -1 && opt[1] == -1;
                                            const bool exact_only = radii != 0 || K == 3 || dmin == 300;
                                            if (exact_only && (shape[0] != 187 || Dd != 64)) continue;
                                            if (radii != 0 && dmin == 300) continue;      // (other radii: any min_disparity > 0 is the volume)
                                            if (cus != 256 && (mode != SMX_MATCH_AUTO || !defaults || sad != 5)) continue;
                                            if (!defaults && (sad != 5 || radii != 0 || K != 2 || mode == SMX_MATCH_EXACT_ORDER)) continue;
                                            if (sad != 5 && Dd != 64) continue;
                                            Config c;
                                            c.default_radii = radii == 0; c.K = K; c.dmin = dmin; c.h = shape[0]; c.w = shape[1]; c.Dd = Dd;
                                            c.B = B; c.match_mode = mode; c.cus = cus; c.sad = sad;
                                            c.opt.fast_dense = opt[0]; c.opt.fast_dense_small = opt[1];
                                            c.exact_filter = cus == 80 ? 1 : (defaults && sad == 5 ? 0 : -1);     // all three values
                                            sweep_facts(c);
                                        }
}

// ---- the directed table ---------------------------------------------------------------------------------------------------
// Written by hand from the rules of enqueue_range as it was before the planner existed; not generated from smx_plan.h.
// C2's pooled 188 x 621, 64 disparities, K 2, 256 CUs, max_batch 64, default radii unless a row says otherwise: a call of
// one pair is "small" (fewer than 13 pairs on a caller's stream, fewer than 8 on the lanes), 32 pairs are not.
static long directed = 0;
static void expect(bool ok, const char *what) {
    ++directed;
    if (!ok) violation("directed: %s", what);
}
static CallFacts call_of(int in_mode, bool on_lanes, bool fast_dense, bool use_filter, int hint) {
    CallFacts call;
    call.in_mode = in_mode; call.on_lanes = on_lanes;
    call.route.fast_dense = fast_dense; call.route.use_filter = use_filter; call.route.grid_hint = hint;
    return call;
}

static void directed_table() {
    Config c2;
    const EngineFacts f = facts_of(c2);
    expect(f.fast_ok && f.default_radii && f.filter_ok && !f.capture && !f.has_volume && f.kt == 2 && f.has_u8_planes() && f.filter_words && f.fast_words,
           "C2 facts");
    for (int whole = 0; whole < 2; ++whole) {
        const bool wc = whole != 0;
        // AUTO, f32 gray, one pair, a caller's stream
        RangePlan p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, -1), 1, wc);
        // (no report yet: the two gated launches; `grid_hint != 0` lets the exact-order one split the range as after an
        // off-grid report)
        expect(p.status == SMX_OK && p.route == AGG_AUTO_GATED && p.mode == SMX_MATCH_AUTO && p.exact_split == wc, "AUTO f32 gray n=1 hint -1: gated");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, 0), 1, wc);
        expect(p.route == AGG_AUTO_ONE_LAUNCH && p.mode == SMX_MATCH_AUTO && !p.exact_split, "AUTO f32 gray n=1 hint 0: one launch");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, 1), 1, wc);
        expect(p.route == AGG_AUTO_GATED && p.exact_split == wc, "AUTO f32 gray n=1 hint 1: gated, split iff whole call");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, 0), 32, wc);
        expect(p.route == AGG_AUTO_GATED && !p.exact_split, "AUTO f32 gray n=32 hint 0: gated, never split");
        for (int hint = -1; hint <= 1; ++hint) {
            p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, hint), 1, wc);
            expect(p.route == AGG_FAST && p.mode == SMX_MATCH_FAST_GRID, "AUTO u8 gray: fast whatever the hint");
        }
        p = plan_range(f, call_of(IN_RGB_U8, false, false, true, -1), 32, wc);
        expect(p.route == AGG_FILTERED && !p.gated_dense_first && p.mode == SMX_MATCH_EXACT_ORDER, "RGB u8 n=32: filtered");
        p = plan_range(f, call_of(IN_RGB_F32, false, false, true, -1), 32, wc);
        expect(p.route == AGG_FILTERED && p.gated_dense_first, "RGB f32 n=32: filtered, gated dense first");
        p = plan_range(f, call_of(IN_RGB_F32, false, false, false, -1), 32, wc);
        expect(p.route == AGG_EXACT && !p.gated_dense_first && p.exact_split == wc, "RGB n=32 without the filter: exact");
        for (int filt = 0; filt < 2; ++filt) {
            p = plan_range(f, call_of(IN_RGB_U8, false, false, filt != 0, -1), 1, wc);
            expect(p.route == AGG_EXACT && p.exact_split == wc, "RGB n=1: exact (small: never filtered), split iff whole call");
        }
        // step 6
        p = plan_range(f, call_of(IN_RGB_F32, false, false, true, -1), 32, wc);
        expect(p.refine_kind == REFINE_FLOAT && p.kt == 2 && p.refine_apron && p.owns_gray, "refine RGB: float, on the engine's aproned planes");
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 4, wc);
        expect(p.refine_kind == REFINE_INT && p.kt == 2 && !p.refine_apron, "refine u8 gray n=4: int");
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 5, wc);
        expect(p.refine_kind == REFINE_INT_V, "refine u8 gray n=5: int_v");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, -1), 4, wc);
        expect(p.refine_kind == REFINE_AUTO && p.refine_reports_grid == wc && !p.owns_gray, "refine f32 gray n=4: auto, reports the grid flag iff whole call");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, -1), 5, wc);
        expect(p.refine_kind == REFINE_AUTO_V && !p.refine_reports_grid, "refine f32 gray n=5: auto_v");
        // fill width
        for (int n : {4, 5, 32})
            for (int lanes = 0; lanes < 2; ++lanes) {
                p = plan_range(f, call_of(IN_GRAY_U8, lanes != 0, false, true, -1), n, wc);
                expect(p.fill_px == (lanes && n > 4 ? 4 : 8), "fill width: 4 iff on the lanes and n > 4");
            }
        // form of the fast kernel, by content: the throughput shape (32 pairs) and the latency shape at 12-row bands (1 pair:
        // 15 windows x 24 bands of 8 rows = 360 workgroups > 256 CUs, 240 of 12 rows fit) have a dense form
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 32, wc);
        expect(!p.fast.small && !p.dense && !p.dense_small && p.reports && p.fill_publishes && p.stride == 8, "fast n=32 sparse: reports, stride 8");
        p = plan_range(f, call_of(IN_GRAY_U8, false, true, true, -1), 32, wc);
        expect(p.dense && !p.dense_small && p.reports && !p.fill_publishes, "fast n=32 dense by content: nothing published");
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 1, wc);
        expect(p.fast.small && p.fast.th == 12 && !p.dense_small && p.reports && p.fill_publishes && p.stride == 1, "fast n=1 sparse: reports, stride 1");
        p = plan_range(f, call_of(IN_GRAY_U8, false, true, true, -1), 1, wc);
        expect(p.dense_small && !p.dense && !p.fill_publishes, "fast n=1 dense by content: the 12-row dense form");
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 6, wc);
        expect(p.fast.small && p.fast.th != 12 && !p.dense && !p.dense_small && !p.reports && !p.fill_publishes, "fast n=6 (8- / 10-row bands): no dense form");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, 0), 1, wc);
        expect(p.route == AGG_AUTO_ONE_LAUNCH && p.reports && p.fill_publishes && p.stride == 1, "one launch n=1 sparse: reports");
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 13, wc);
        expect(!p.fast.small && p.stride == 4, "fast n=13: stride (n + 3) / 4");
    }
    {   // forced forms
        Config c = c2;
        c.opt.fast_dense = 1;
        EngineFacts ff = facts_of(c);
        RangePlan p = plan_range(ff, call_of(IN_GRAY_U8, false, true, true, -1), 32, true);
        expect(p.dense && !p.reports && !p.fill_publishes, "SMX_FAST_DENSE=1 n=32: dense, never reports");
        p = plan_range(ff, call_of(IN_GRAY_U8, false, true, true, -1), 1, true);
        expect(p.dense_small && !p.reports && !p.fill_publishes, "SMX_FAST_DENSE=1 n=1: dense, never reports");
        c.opt.fast_dense = 0;
        ff = facts_of(c);
        p = plan_range(ff, call_of(IN_GRAY_U8, false, false, true, -1), 32, true);
        expect(!p.dense && !p.reports && !p.fill_publishes, "SMX_FAST_DENSE=0 n=32: sparse, never reports");
        c.opt.fast_dense = -1;
        c.opt.fast_dense_small = 1;
        ff = facts_of(c);
        p = plan_range(ff, call_of(IN_GRAY_U8, false, false, true, -1), 1, true);
        expect(p.dense_small && !p.reports && !p.fill_publishes, "SMX_FAST_DENSE_SMALL=1 n=1: dense whatever the content");
        c.opt.fast_dense_small = 0;
        ff = facts_of(c);
        p = plan_range(ff, call_of(IN_GRAY_U8, false, true, true, -1), 1, true);
        expect(!p.dense_small && !p.dense && p.reports && p.fill_publishes, "SMX_FAST_DENSE_SMALL=0 n=1: sparse whatever the content");
    }
    {   // min_disparity > 0 on the capture route: the same routes, each followed by its lookups; one launch never
        Config c = c2;
        c.dmin = 8;
        const EngineFacts fc = facts_of(c);
        expect(fc.capture && !fc.has_volume && fc.filter_ok, "capture facts");
        RangePlan p = plan_range(fc, call_of(IN_GRAY_F32, false, false, true, 0), 1, true);
        expect(p.route == AGG_AUTO_GATED && p.capture_follows && !p.exact_split, "capture, AUTO f32 gray n=1 hint 0: gated, not one launch");
        p = plan_range(fc, call_of(IN_GRAY_F32, false, false, true, 1), 1, true);
        expect(p.route == AGG_AUTO_GATED && p.capture_follows && p.exact_split, "capture, hint 1: gated with the split");
        p = plan_range(fc, call_of(IN_GRAY_U8, false, true, true, -1), 32, true);
        expect(p.route == AGG_FAST && p.capture_follows && !p.dense && !p.dense_small && !p.reports && !p.fill_publishes, "capture, u8 gray: fast, no dense form");
        p = plan_range(fc, call_of(IN_GRAY_U8, false, true, true, -1), 1, true);
        expect(p.route == AGG_FAST && !p.dense_small && !p.reports, "capture, u8 gray n=1: no dense form");
        p = plan_range(fc, call_of(IN_RGB_F32, false, false, true, -1), 32, true);
        expect(p.route == AGG_FILTERED && p.gated_dense_first && p.capture_follows, "capture, RGB f32 n=32: filtered");
        p = plan_range(fc, call_of(IN_RGB_U8, false, false, false, -1), 32, true);
        expect(p.route == AGG_EXACT && p.capture_follows, "capture, RGB n=32 without the filter: exact");
    }
    {   // other radii with min_disparity > 0: the aggregated volume
        Config c = c2;
        c.default_radii = false;
        c.dmin = 8;
        EngineFacts fv = facts_of(c);
        expect(fv.has_volume && !fv.capture && !fv.filter_ok && !fv.fast_ok, "volume facts");
        for (int in_mode : {IN_GRAY_F32, IN_RGB_F32, IN_GRAY_U8, IN_RGB_U8}) {
            const RangePlan p = plan_range(fv, call_of(in_mode, false, false, true, 0), 1, true);
            expect(p.status == SMX_OK && p.route == AGG_EXACT && p.mode == SMX_MATCH_EXACT_ORDER && !p.capture_follows && p.exact_split, "volume, AUTO: exact");
        }
        c.match_mode = SMX_MATCH_FAST_GRID;
        fv = facts_of(c);
        expect(plan_range(fv, call_of(IN_GRAY_U8, false, false, true, -1), 1, true).status == SMX_ERR_UNSUPPORTED, "volume, FAST_GRID: refused");
        c = c2;
        c.dmin = 300;                       // default radii, min_disparity / K beyond the disparity count: the volume as well
        c.match_mode = SMX_MATCH_FAST_GRID;
        fv = facts_of(c);
        expect(fv.has_volume && fv.fast_ok && plan_range(fv, call_of(IN_GRAY_U8, false, false, true, -1), 1, true).status == SMX_ERR_UNSUPPORTED,
               "default radii, volume, FAST_GRID: refused");
        const CallKind k = call_kind(fv, IN_GRAY_U8, false, 32, 0);
        expect(!k.fast_reports && !k.filter_reports, "a refused call reports to no switch");
    }
    {   // K = 3: off the exact grid
        Config c = c2;
        c.K = 3;
        c.match_mode = SMX_MATCH_FAST_GRID;
        EngineFacts f3 = facts_of(c);
        expect(!f3.fast_ok && !f3.grid_capable && plan_range(f3, call_of(IN_GRAY_F32, false, false, true, -1), 1, true).status == SMX_ERR_UNSUPPORTED,
               "K = 3, FAST_GRID: refused");
        c.match_mode = SMX_MATCH_AUTO;
        f3 = facts_of(c);
        const RangePlan p = plan_range(f3, call_of(IN_GRAY_U8, false, false, true, -1), 1, true);
        expect(p.status == SMX_OK && p.route == AGG_EXACT && p.refine_kind == REFINE_FLOAT && p.kt == 0, "K = 3, AUTO: exact, generic step 6");
    }
    {   // sad_patch_radius 4: the generic float step-6 kernel, whatever the entry
        Config c = c2;
        c.sad = 4;
        const EngineFacts f4 = facts_of(c);
        for (int in_mode : {IN_GRAY_F32, IN_RGB_F32, IN_GRAY_U8, IN_RGB_U8}) {
            const RangePlan p = plan_range(f4, call_of(in_mode, false, false, true, -1), 4, true);
            expect(p.refine_kind == REFINE_FLOAT && p.kt == 0 && !p.refine_apron && !p.refine_reports_grid, "sad_patch_radius 4: float, kt 0");
        }
    }
    {   // the prediction on the table's shape
        CallKind k = call_kind(f, IN_RGB_U8, false, 32, 0);
        expect(k.filter_reports && !k.fast_reports, "kind: RGB n=32 reports to the filter switch");
        k = call_kind(f, IN_RGB_U8, false, 1, 0);
        expect(!k.filter_reports && !k.fast_reports, "kind: RGB n=1 reports to neither");
        k = call_kind(f, IN_GRAY_F32, true, 16, 16);
        expect(!k.filter_reports && k.fast_reports, "kind: gray halves of 16 report to the fast switch");
        k = call_kind(f, IN_GRAY_U8, false, 6, 0);
        expect(!k.filter_reports && !k.fast_reports, "kind: gray n=6 (short bands) reports to neither");
    }
}

int main() {
    directed_table();
    sweep();
    printf("launch-plan plans %ld kinds %ld directed %ld routes %ld %ld %ld %ld %ld refused %ld refine %ld %ld %ld %ld %ld hash %016llx violations %ld\n",
           plans, kinds, directed, routes[AGG_FILTERED], routes[AGG_EXACT], routes[AGG_FAST], routes[AGG_AUTO_ONE_LAUNCH], routes[AGG_AUTO_GATED],
           refused, refines[REFINE_FLOAT], refines[REFINE_INT], refines[REFINE_INT_V], refines[REFINE_AUTO], refines[REFINE_AUTO_V], plan_hash, violations);
    return violations == 0 ? 0 : 1;
}
