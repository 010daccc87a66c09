// Host-only harness of tests/test_launch_plan_cpu.py: the engine's launch planner (stereo-depth_amd/csrc/smx_plan.h) against
// its own prediction, its invariants and a table written by hand.  It compiles the lines the engine runs and never calls
// the HIP runtime.
//
//   1. Prediction equals execution.  call_kind() tells the content switches whether a call's default route holds a launch
//      that reports to them; the right-hand side is evaluated here from the RangePlan fields enqueue_range reads.
//   2. Plan invariants, over the sweep (configurations x match modes x entries x lanes x pairs x halves x decisions x
//      forced options x CU counts).
//   3. The directed table: the plans of today's rules for the cases a reader would ask about first.
//   4. The launch specs.  Every aggregation launch a plan names (ExactLaunch, ExactCaptureLaunch, FastLaunch,
//      FastCaptureLaunch, AutoLaunch, FilterLaunch) against the launcher glue as it was while the launchers still decided
//      for themselves, restated here by hand (old_*), field by field over the whole sweep; and the specs' own invariants:
//      a split fits the lane's slice region and belongs to a whole call of at most 4 pairs, a dense form is planned only
//      where its instantiation exists, the dynamic LDS stays within what the engine raises the kernel to.  A call planned
//      dense that launches the sparse instantiation (no dense one exists for it) is counted: "dense-fallback".
//   5. The rest of the call.  PrologueLaunch, RefineLaunch and FillLaunch against launch_prologue's and launch_fill's own
//      selection and enqueue_range's sad_exact and log2k as they were while those decided for themselves; the gates and
//      the MatchParams of every aggregation launch (smx_plan.h: exact_params, ..., auto_params) against the four lambdas
//      enqueue_range had, all restated here by hand (old_*), field by field over the whole sweep.  The prologue also
//      with the caller's u8 pointers unaligned, and an extension of the sweep (K = 8; widths that are no multiple of
//      K) that is checked and hashed like the rest but stays out of the counts and the first hash.  Invariants: the
//      K = 2 prologue only for gray entries with even W, the K = 4 prologue only with grid_capable, W % 4 == 0 and
//      aligned u8 input; integer step-6 kinds only with kt != 0 and u8 planes; sad_exact false exactly beyond the
//      bound; a split launch has nsplit == split, pairs == n and no tickets; of a gated pair exactly one launch runs
//      for either value of the flag.
//
// Output: a line per violation ("violation <what>: <inputs>", the first 60), then
//   "launch-plan plans <n> kinds <n> directed <n> routes <FILTERED> <EXACT> <FAST> <AUTO_ONE_LAUNCH> <AUTO_GATED> refused <n>
//    refine <FLOAT> <INT> <INT_V> <AUTO> <AUTO_V> hash <fnv-1a of every (inputs -> plan) of the sweep> violations <n>
//    specs <launch specs compared> exact <GENERIC> <GENERIC_VOLUME> <TILED> split <exact launches split> form <SPARSE>
//    <PASS1_ONLY> <DENSE> <DENSE_SMALL> dense-fallback <n> hash2 <fnv-1a of the fields of item 5> prologue <GENERIC> <K2> <K4>
//    fill <FILL_4> <POW2> <GENERIC> sx0 <plans whose step 6 evaluates the parabola> params <MatchParams compared>".
//  `hash` covers the fields it covered before item 5 existed (it does not move when only those are added); `hash2` the rest.
//
// Other uses (tests/test_launch_spec_gpu.py), on the CU count given:
//   launch_plan_harness spec <cus> <radii> <K> <h> <w> <Dd> <dmin> <B> <mode> <opt dense> <opt dense small> <in_mode> <lanes>
//                       <dense> <filter> <hint> <n> <whole> <crop> <aligned>
//                                                                one line "keys ..." : the spec keys of that plan
//                       (crop: W = K * w - crop; aligned: the caller's u8 pointers)
//   launch_plan_harness reach <cus>                              "reach-small ..." / "reach-large-only ...": the keys the
//                       sweep's configurations reach at its two smallest shapes, and those only its larger shapes reach
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>

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
    int crop = 0;                   // W = K * w - crop (< K): a width that is no multiple of K
    int match_mode = SMX_MATCH_AUTO, exact_filter = 0, cus = 256;
    PlanOptions opt;
};

static EngineFacts facts_of(const Config &c) {
    smx_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.height = (unsigned)(c.h * c.K); cfg.width = (unsigned)(c.w * c.K - c.crop); cfg.downscale_factor = (unsigned)c.K;
    cfg.min_disparity = c.dmin * c.K; cfg.max_disparity = (c.dmin + c.Dd) * c.K - 1;
    cfg.ncc_patch_radius = 1; cfg.sad_patch_radius = (unsigned)c.sad; cfg.threshold = 5;
    cfg.small_mbm_radius = c.default_radii ? 1 : 2; cfg.mid_mbm_radius = c.default_radii ? 4 : 3; cfg.large_mbm_radius = c.default_radii ? 10 : 8;
    cfg.max_batch = c.B; cfg.match_mode = c.match_mode; cfg.exact_filter = c.exact_filter;
    smx_dims d;
    d.H = c.h * c.K; d.W = c.w * c.K - c.crop; d.K = c.K; d.h = c.h; d.w = c.w; d.dmin = c.dmin; d.dmax = c.dmin + c.Dd - 1; d.Dd = c.Dd;
    return derive_facts(cfg, d, c.cus, c.opt);
}

static const char *describe(const Config &c, const CallFacts &call, int n, bool whole) {
    static char buf[256];
    snprintf(buf, sizeof(buf), "radii %d K %d %dx%d crop %d Dd %d dmin %d sad %d B %d mode %d filter %d cus %d opt %d %d | in %d al %d lanes %d dense %d filt %d hint %d | n %d whole %d",
             c.default_radii ? 1 : 0, c.K, c.h, c.w, c.crop, c.Dd, c.dmin, c.sad, c.B, c.match_mode, c.exact_filter, c.cus, c.opt.fast_dense, c.opt.fast_dense_small,
             call.in_mode, call.u8_aligned ? 1 : 0, call.on_lanes ? 1 : 0, call.route.fast_dense ? 1 : 0, call.route.use_filter ? 1 : 0, call.route.grid_hint, n, whole ? 1 : 0);
    return buf;
}

// ---- the launcher glue of the parent, restated ---------------------------------------------------------------------------
// Written by hand from tu_exact.hip, tu_fast_small.hip and the launcher tails of k_match_fast.h, k_match_auto.h,
// k_match_capture.h and k_match_filter.h as they were when each launcher took (params, n, cus) and chose its instantiation
// itself; not built by calling the spec functions of smx_plan.h.  `p` is the MatchParams enqueue_range handed them.
static MatchParams engine_params(const Config &c, const EngineFacts &f, const RangePlan &pl, bool on_lanes) {
    MatchParams p{};
    p.B = f.B; p.h = f.h; p.w = f.w; p.dmin = f.dmin; p.Dd = f.Dd;
    p.rn = 1; p.rs = c.default_radii ? 1 : 2; p.rm = c.default_radii ? 4 : 3; p.rl = c.default_radii ? 10 : 8;
    p.unit = (float)(c.K * c.K);
    p.on_lanes = on_lanes ? 1 : 0;
    p.pass1_only = pl.capture_follows ? 1 : 0;
    return p;
}
struct OldExact { int kernel, split, rows, nd_chunk; size_t lds, need; };
static OldExact old_launch_exact(const EngineFacts &f, MatchParams p, bool vol, int n, bool allow_split, int cus) {
    if (!vol && p.rn == 1 && p.rs == 1 && p.rm == 4 && p.rl == 10) {
        const int gx = (p.w + E2_TW - 1) / E2_TW, gy = (p.h + E2_TH - 1) / E2_TH;
        p.nd_chunk = f.exact2_nd;
        const int sp = allow_split ? exact_split(gx * gy, n, p.Dd, cus) : 1;
        if (sp > 1) {
            const size_t need = (size_t)sp * SMX_SLICE_WORDS * n * p.h * p.w;
            const int gz = n * sp;
            const int per = (p.Dd + sp - 1) / sp;
            if (p.nd_chunk > per) p.nd_chunk = per;
            const long wgs = (long)gx * gy * gz, slots = 2L * cus;
            const int rows = (p.on_lanes && 2 * wgs > slots && wgs < 2 * slots) ? 4 : 2;
            return OldExact{EXACT_TILED, sp, rows, p.nd_chunk, f.exact2_lds, need};
        }
        return OldExact{EXACT_TILED, 1, 4, p.nd_chunk, f.exact2_lds, 0};
    }
    return OldExact{vol ? EXACT_GENERIC_VOLUME : EXACT_GENERIC, 1, 4, f.exact_nd, f.exact_lds, 0};
}
// (capture_split was a static function of tu_exact.hip: its body is the one now in k_match_exact2.h, restated too)
static int old_capture_split(int tiles, int n, int Dd, int cus) {
    if (n > 4 || Dd < 16) return 1;
    const long slots = 2L * cus, wgs = (long)tiles * n, need = (Dd + 3) / 4;
    int best = 1;
    long best_cost = ((wgs + slots - 1) / slots) * (2 + need);
    for (int sp = 2; sp <= 8; ++sp) {
        const long cost = ((wgs * sp + slots - 1) / slots) * (2 + (need + sp - 1) / sp);
        if (cost < best_cost) { best_cost = cost; best = sp; }
    }
    return best;
}
static ExactCaptureLaunch old_launch_exact2_capture(const EngineFacts &f, const MatchParams &cp, int n, bool allow_split, int cus) {
    const int gx = (cp.w + E2_TW - 1) / E2_TW, gy = (cp.h + E2_TH - 1) / E2_TH;
    ExactCaptureLaunch x;
    x.nd_chunk = f.exact2_nd;
    x.split = allow_split ? old_capture_split(gx * gy, n, cp.Dd, cus) : 1;
    x.rows_per_thread = allow_split ? 2 : 4;
    x.lds_bytes = f.exact2_lds + E2_CAPBITS * sizeof(unsigned);
    return x;
}
static FastLaunch old_launch_match_fast(const MatchParams &p, int n, int cus) {
    const FastPlan pl = match_fast_plan(p, n, cus);
    FastLaunch x;
    bool dsplit;
    if (pl.small) {                                              // launch_match_fast_t<TH, 256 / 320, true>
        x.th = pl.th == FA_TH_SMALL_TALL ? FA_TH_SMALL_TALL : (pl.th == FA_TH_SMALL_MID ? FA_TH_SMALL_MID : FA_TH_SMALL);
        x.pitch = !pl.wide ? 256 : 320;
        dsplit = true;
        x.argb = false;                                          // launch_match_fast_a<TH, PR, true, false>
    } else {
        if (pl.th == 27 || (pl.th == 32 && p.dense && !p.pass1_only && p.Dd <= 256)) x.th = 27;
        else if (pl.th == 32) x.th = 32;
        else x.th = 24;
        x.pitch = fast_tall_pitch(p.Dd);                         // launch_match_fast_tall<TH>
        dsplit = false;
        x.argb = (x.pitch == 256 || x.pitch == FA_MID_PITCH) ? true : p.Dd <= 256;
    }
    x.small = dsplit;
    x.pk = p.unit <= 4.0f ? 2 : (p.unit <= 16.0f ? 1 : 0);       // launch_match_fast_a
    if (dsplit && x.th == FA_TH_SMALL_TALL && p.dense_small && !p.pass1_only && p.Dd <= x.pitch - 64 + 1) x.form = FAST_DENSE_SMALL;
    else if (!dsplit && x.argb && x.th <= FA_DENSE_MAX_TH && p.dense && !p.pass1_only) x.form = FAST_DENSE;
    else if (p.pass1_only) x.form = FAST_PASS1_ONLY;
    else x.form = FAST_SPARSE;
    return x;
}
static FastCaptureLaunch old_launch_match_capture(const MatchParams &p, int n, int cus) {
    FastCaptureLaunch x;
    x.wide = p.Dd > FA_WIDE_FROM;
    x.small = match_fast_plan(p, n, cus).small;
    x.pk = p.unit <= 4.0f ? 2 : (p.unit <= 16.0f ? 1 : 0);
    return x;
}
static AutoLaunch old_launch_match_auto_small(const EngineFacts &f, MatchParams p, int n, int cus) {
    AutoLaunch x;
    x.th = match_fast_plan(p, n, cus).th;                        // launch_match_auto_small_tu
    p.nd_chunk = f.exact2_nd;                                    // (enqueue_range)
    x.wide = p.Dd > 256 - 64 + 1;
    size_t lds = x.wide ? fast_lds_bytes<320>(x.th, p.Dd, true) : fast_lds_bytes<256>(x.th, p.Dd, true);
    p.nsplit = match_auto_nsplit(p, x.th);
    const int per = (p.Dd + p.nsplit - 1) / p.nsplit;
    if (p.nd_chunk > per) p.nd_chunk = per;
    const size_t exact_lds = exact2_lds_floats(p.nd_chunk) * sizeof(float);
    if (exact_lds > lds) lds = exact_lds;
    x.nsplit = p.nsplit; x.nd_chunk = p.nd_chunk; x.lds_bytes = lds;
    x.pk = p.unit <= 4.0f ? 2 : (p.unit <= 16.0f ? 1 : 0);
    return x;
}
static FilterLaunch old_launch_match_filter(const EngineFacts &f, MatchParams p, int n, int cus) {
    p.unit = (float)f.filter_unit;                               // (enqueue_range: fmp)
    const FilterPlan pl = filter_plan(p, n, cus);
    return FilterLaunch{pl.th, pl.wide, p.unit <= 4.0f ? 2 : (p.unit <= 16.0f ? 1 : 0)};
}

// ---- the glue around the specs of item 5, restated -------------------------------------------------------------------------
// Written by hand from tu_stages.hip (launch_prologue / prologue_t, launch_fill) and from enqueue_range of smx_engine.hip as
// they were while they decided for themselves; not built by calling smx_plan.h.
static int old_launch_prologue(int in_mode, const Config &c, const EngineFacts &f, bool aligned) {
    const int K = c.K, W = c.w * c.K - c.crop;                   // PrologueArgs as enqueue_range filled them
    const int grid_capable = f.grid_capable ? 1 : 0, pitch8 = f.pitch8, padl = f.padl, gpitch = f.gpitch, gpadl = f.gpadl;
    if ((in_mode == IN_GRAY_F32 || in_mode == IN_GRAY_U8) && K == 2 && (W & 1) == 0) return PROLOGUE_K2;
    const bool U8IN = in_mode == IN_GRAY_U8 || in_mode == IN_RGB_U8;
    if (K == 4 && (W & 3) == 0 && grid_capable && (gpitch & 3) == 0 && (gpadl & 3) == 0 && (pitch8 & 3) == 0 && (padl & 3) == 0 &&
        (gpadl == 0 || gpadl == padl) && (!U8IN || aligned))
        return PROLOGUE_K4;
    return PROLOGUE_GENERIC;
}
struct FillInst { int kernel, K, px; };                          // k_fill4<K, px> or k_fill<pow2> (K, px 0)
static FillInst old_launch_fill(int K, int px) {
    const bool pow2 = (K & (K - 1)) == 0;
    if (K == 1) return FillInst{FILL_4, 1, 4};
    else if (K == 2 && px == 4) return FillInst{FILL_4, 2, 4};
    else if (K == 2) return FillInst{FILL_4, 2, 8};
    else if (K == 4 && px == 4) return FillInst{FILL_4, 4, 4};
    else if (K == 4) return FillInst{FILL_4, 4, 8};
    else if (pow2) return FillInst{FILL_POW2, 0, 0};
    return FillInst{FILL_GENERIC, 0, 0};
}
static FillInst fill_inst(const FillLaunch &x) {                 // the instantiation the table of launch_fill names for a spec
    if (x.kernel != FILL_4) return FillInst{x.kernel, 0, 0};
    return FillInst{FILL_4, x.K, x.K == 1 ? 4 : x.px};
}
// enqueue_range's aggregation part: the shared MatchParams `mp`, the four lambdas and the switch over the route, with every
// launch replaced by a record of the MatchParams it was handed
static int dummy_flags[1], dummy_flags2[1];
static unsigned dummy_tickets[1];
static unsigned long long dummy_stats[1];
static float dummy_f[1];
struct OldParams { MatchParams exact, exact_capture, fast, fast_capture, auto_small, filter, sparse; };
static OldParams old_enqueue_range(const EngineFacts &f, const RangePlan &pl, MatchParams mp, int n) {
    OldParams o{};
    auto exact_capture = [&](MatchParams p) {
        if (!pl.capture_follows) return;
        p.nd_chunk = pl.exact_capture.nd_chunk;
        p.nsplit = pl.exact_capture.split;
        o.exact_capture = p;
    };
    auto exact = [&](MatchParams p) {
        p.nd_chunk = pl.exact.nd_chunk;
        if (pl.exact.split > 1) {
            p.nsplit = pl.exact.split;
            p.pairs = n;
            p.tickets = nullptr;
        }
        o.exact = p;
    };
    auto fast_params = [&](MatchParams p, int gate) -> MatchParams {
        p.gate = gate;
        p.dense = pl.dense ? 1 : 0;
        p.dense_small = pl.dense_small ? 1 : 0;
        if (pl.fill_publishes) {
            p.fast_stats = dummy_stats;
            p.fast_stride = pl.stride;
        }
        return p;
    };
    auto fast = [&](int gate) {
        const MatchParams p = fast_params(mp, gate);
        o.fast = p;
        if (pl.capture_follows) o.fast_capture = p;
    };
    switch (pl.route) {
    case AGG_FILTERED: {
        if (pl.gated_dense_first) {
            MatchParams dp = mp;
            dp.flags = dummy_flags2;
            dp.gate = 2;
            exact(dp);
        }
        MatchParams fmp = mp;
        fmp.unit = (float)f.filter_unit;
        o.filter = fmp;
        MatchParams sp = mp;
        sp.nd_chunk = f.exact2_nd;
        o.sparse = sp;
        exact_capture(mp);
        break;
    }
    case AGG_EXACT:
        exact(mp);
        exact_capture(mp);
        break;
    case AGG_FAST: fast(0); break;
    case AGG_AUTO_ONE_LAUNCH: {
        MatchParams p = fast_params(mp, 0);
        p.nsplit = pl.auto_launch.nsplit;
        p.pairs = n;
        p.nd_chunk = pl.auto_launch.nd_chunk;
        o.auto_small = p;
        break;
    }
    default:
        mp.gate = 2;
        exact(mp);
        exact_capture(mp);
        fast(1);
        break;
    }
    return o;
}
static bool same_params(const MatchParams &a, const MatchParams &b) {
    return a.Ld == b.Ld && a.Rd == b.Rd && a.wta == b.wta && a.costs == b.costs && a.vol == b.vol && a.flags == b.flags && a.epoch == b.epoch &&
           a.B == b.B && a.h == b.h && a.w == b.w && a.dmin == b.dmin && a.Dd == b.Dd && a.rn == b.rn && a.rs == b.rs && a.rm == b.rm && a.rl == b.rl &&
           a.gate == b.gate && a.nd_chunk == b.nd_chunk && a.unit == b.unit && a.nsplit == b.nsplit && a.pairs == b.pairs && a.slices == b.slices &&
           a.pass1_only == b.pass1_only && a.dense == b.dense && a.dense_small == b.dense_small && a.fast_stats == b.fast_stats &&
           a.fast_stride == b.fast_stride && a.on_lanes == b.on_lanes && a.tickets == b.tickets;
}
static bool gate_runs(int gate, bool flag) { return gate == 0 || (gate == 1 && !flag) || (gate == 2 && flag); }    // MatchParams::gate

static const char *const ENTRY_NAMES[] = {"gray_f32", "rgb_f32", "gray_u8", "rgb_u8"};
static const char *const PROLOGUE_NAMES[] = {"generic", "k2", "k4"};
static const char *const REFINE_NAMES[] = {"FLOAT", "INT", "INT_V", "AUTO", "AUTO_V"};
static const char *const FILL_NAMES[] = {"fill4", "pow2", "generic"};
static const char *const EXACT_NAMES[] = {"GENERIC", "GENERIC_VOLUME", "TILED"};
static const char *const FORM_NAMES[] = {"SPARSE", "PASS1_ONLY", "DENSE", "DENSE_SMALL"};
static bool has_exact(const RangePlan &p) { return (p.route == AGG_FILTERED && p.gated_dense_first) || p.route == AGG_EXACT || p.route == AGG_AUTO_GATED; }
static bool has_exact_capture(const RangePlan &p) { return p.capture_follows && (p.route == AGG_FILTERED || p.route == AGG_EXACT || p.route == AGG_AUTO_GATED); }
static bool has_fast(const RangePlan &p) { return p.route == AGG_FAST || p.route == AGG_AUTO_GATED; }

// The spec keys of a plan: one "<spec>.<field>=<value>" per field that selects an instantiation, of the launches it enqueues.
static void keys_of(const RangePlan &p, std::set<std::string> &keys) {
    char b[64];
    auto key = [&](const char *fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(b, sizeof(b), fmt, ap);
        va_end(ap);
        keys.insert(b);
    };
    if (has_exact(p)) {
        key("exact.kernel=%s", EXACT_NAMES[p.exact.kernel]);
        if (p.exact.kernel == EXACT_TILED) key(p.exact.split > 1 ? "exact.split=yes.rows=%d" : "exact.split=no", p.exact.rows_per_thread);
    }
    if (has_exact_capture(p)) key("exact_capture.rows=%d", p.exact_capture.rows_per_thread);
    if (has_fast(p)) {
        key("fast.form=%s", FORM_NAMES[p.fast_launch.form]);
        key("fast.small=%d.th=%d", p.fast_launch.small ? 1 : 0, p.fast_launch.th);
        key("fast.small=%d.pitch=%d", p.fast_launch.small ? 1 : 0, p.fast_launch.pitch);
        key("fast.pk=%d", p.fast_launch.pk);
        if (!p.fast_launch.small) key("fast.argb=%d", p.fast_launch.argb ? 1 : 0);
        if (p.capture_follows) key("fast_capture.small=%d.wide=%d", p.fast_capture.small ? 1 : 0, p.fast_capture.wide ? 1 : 0);
    }
    if (p.route == AGG_AUTO_ONE_LAUNCH) key("auto.th=%d.wide=%d", p.auto_launch.th, p.auto_launch.wide ? 1 : 0);
    if (p.route == AGG_FILTERED) key("filter.th=%d.wide=%d", p.filter.th, p.filter.wide ? 1 : 0);
    // (a field the table does not look at for the row is printed as the row's only value)
    key("prologue.%s.%s", ENTRY_NAMES[p.prologue.in_mode], PROLOGUE_NAMES[p.prologue.kernel]);
    key("refine.%s.kt=%d.apron=%d.sx=%d", REFINE_NAMES[p.refine.kind], p.refine.kt, p.refine.kind == REFINE_FLOAT && p.refine.apron ? 1 : 0,
        p.refine.kind == REFINE_FLOAT || p.refine.sad_exact ? 1 : 0);
    const FillInst fi = fill_inst(p.fill);
    key("fill.%s.k=%d.px=%d", FILL_NAMES[fi.kernel], fi.K, fi.px);
}
static std::set<std::string> *reach_keys = nullptr;                 // `reach`: collect instead of checking

// ---- the sweep -----------------------------------------------------------------------------------------------------------
static unsigned long long plan_hash = 1469598103934665603ull;
static void mix(long long v) {
    for (int i = 0; i < 8; ++i) {
        plan_hash ^= (unsigned long long)(v >> (8 * i)) & 0xffull;
        plan_hash *= 1099511628211ull;
    }
}
static unsigned long long plan_hash2 = 1469598103934665603ull;
static void mix2(long long v) {
    for (int i = 0; i < 8; ++i) {
        plan_hash2 ^= (unsigned long long)(v >> (8 * i)) & 0xffull;
        plan_hash2 *= 1099511628211ull;
    }
}
static bool extension = false;      // the sweep's extension (item 5): checked and hashed into hash2; not in the first hash nor in the counts before hash2
static long prologues[3] = {}, fills[3] = {}, sx0 = 0, params_compared = 0;
static long plans = 0, kinds = 0, refused = 0, routes[AGG_ROUTES] = {}, refines[5] = {};
static long specs = 0, exact_kernels[3] = {}, exact_splits = 0, forms[FAST_FORMS] = {}, dense_fallbacks = 0;

// item 4 of the head comment
static void check_specs(const Config &c, const EngineFacts &f, const CallFacts &call, const RangePlan &p, int n, bool whole) {
#define SPEC_EQ(what, a, b) do { if ((long long)(a) != (long long)(b)) violation("spec %s: %lld, the parent's launcher %lld: %s", what, (long long)(a), (long long)(b), describe(c, call, n, whole)); } while (0)
    MatchParams mp = engine_params(c, f, p, call.on_lanes);
    const size_t tiled_cap = (size_t)SMX_EXACT2_LDS_CAP + (E2_CAPBITS + 2 * E2_SPARSE_WORDS) * sizeof(unsigned);    // smx_engine.hip: raise_lds_caps
    if (has_exact(p)) {
        // (the gated dense launch of the filtered route never splits; the others as the plan allows)
        const OldExact o = old_launch_exact(f, mp, f.has_volume, n, p.route == AGG_FILTERED ? false : p.exact_split, f.cus);
        if (!extension) ++specs;
        if (!extension) exact_kernels[p.exact.kernel]++;
        if (p.exact.split > 1 && !extension) ++exact_splits;
        SPEC_EQ("exact.kernel", p.exact.kernel, o.kernel);
        SPEC_EQ("exact.split", p.exact.split, o.split);
        SPEC_EQ("exact.rows_per_thread", p.exact.rows_per_thread, o.rows);
        SPEC_EQ("exact.nd_chunk", p.exact.nd_chunk, o.nd_chunk);
        SPEC_EQ("exact.lds_bytes", p.exact.lds_bytes, o.lds);
        SPEC_EQ("exact.slice_floats", p.exact.slice_floats, o.need);
        if (p.exact.split < 1 || p.exact.split > 8 || (p.exact.rows_per_thread != 2 && p.exact.rows_per_thread != 4) || p.exact.nd_chunk < 1)
            violation("exact spec out of range: %s", describe(c, call, n, whole));
        if (p.exact.split > 1 && p.exact.slice_floats > f.slices_floats) violation("split does not fit the lane's slice region: %s", describe(c, call, n, whole));
        if ((p.exact.split > 1) != (p.exact.slice_floats != 0)) violation("slice floats without a split: %s", describe(c, call, n, whole));
        if (p.exact.split > 1 && (!whole || n > 4)) violation("split outside whole calls of at most 4 pairs: %s", describe(c, call, n, whole));
        if (p.exact.lds_bytes > (p.exact.kernel == EXACT_TILED ? tiled_cap : (size_t)64 * 1024)) violation("exact LDS beyond the cap: %s", describe(c, call, n, whole));
    }
    if (has_exact_capture(p)) {
        const ExactCaptureLaunch o = old_launch_exact2_capture(f, mp, n, p.route == AGG_FILTERED ? false : p.exact_split, f.cus);
        if (!extension) ++specs;
        SPEC_EQ("exact_capture.split", p.exact_capture.split, o.split);
        SPEC_EQ("exact_capture.rows_per_thread", p.exact_capture.rows_per_thread, o.rows_per_thread);
        SPEC_EQ("exact_capture.nd_chunk", p.exact_capture.nd_chunk, o.nd_chunk);
        SPEC_EQ("exact_capture.lds_bytes", p.exact_capture.lds_bytes, o.lds_bytes);
        if (p.exact_capture.split > 1 && (!whole || n > 4)) violation("capture split outside whole calls of at most 4 pairs: %s", describe(c, call, n, whole));
        if (p.exact_capture.split < 1 || p.exact_capture.split > 8 || p.exact_capture.lds_bytes > tiled_cap) violation("exact capture spec: %s", describe(c, call, n, whole));
    }
    if (has_fast(p)) {
        mp.dense = p.dense ? 1 : 0;                               // (enqueue_range: fast())
        mp.dense_small = p.dense_small ? 1 : 0;
        const FastLaunch o = old_launch_match_fast(mp, n, f.cus), &x = p.fast_launch;
        if (!extension) ++specs;
        if (!extension) forms[x.form]++;
        SPEC_EQ("fast.th", x.th, o.th);
        SPEC_EQ("fast.small", x.small, o.small);
        SPEC_EQ("fast.pitch", x.pitch, o.pitch);
        SPEC_EQ("fast.pk", x.pk, o.pk);
        SPEC_EQ("fast.argb", x.argb, o.argb);
        SPEC_EQ("fast.form", x.form, o.form);
        // the instantiations that exist (k_match_fast.h: launch_match_fast_a / _t, the three tall translation units)
        const bool shape_ok = x.small ? ((x.th == 8 || x.th == 10 || x.th == 12) && (x.pitch == 256 || x.pitch == 320) && !x.argb)
                                      : ((x.th == 24 || x.th == 27 || x.th == 32) && (x.pitch == 256 || x.pitch == FA_MID_PITCH || x.pitch == 320) &&
                                         (x.argb || x.pitch == 320));
        if (!shape_ok || x.pk < 0 || x.pk > 2) violation("fast spec names no instantiation: %s", describe(c, call, n, whole));
        if (x.form == FAST_DENSE && (x.small || !x.argb || x.th > FA_DENSE_MAX_TH || f.Dd > 256)) violation("DENSE without an instantiation: %s", describe(c, call, n, whole));
        if (x.form == FAST_DENSE_SMALL && (!x.small || x.th != FA_TH_SMALL_TALL || f.Dd > x.pitch - 64 + 1)) violation("DENSE_SMALL without an instantiation: %s", describe(c, call, n, whole));
        if ((x.form == FAST_PASS1_ONLY) != f.capture) violation("PASS1_ONLY: %s", describe(c, call, n, whole));
        if ((x.form == FAST_DENSE && !p.dense) || (x.form == FAST_DENSE_SMALL && !p.dense_small)) violation("dense form not planned: %s", describe(c, call, n, whole));
        if ((p.dense || p.dense_small) && x.form == FAST_SPARSE && !extension) ++dense_fallbacks;
        if (p.capture_follows) {
            const FastCaptureLaunch oc = old_launch_match_capture(mp, n, f.cus);
            if (!extension) ++specs;
            SPEC_EQ("fast_capture.small", p.fast_capture.small, oc.small);
            SPEC_EQ("fast_capture.wide", p.fast_capture.wide, oc.wide);
            SPEC_EQ("fast_capture.pk", p.fast_capture.pk, oc.pk);
        }
    }
    if (p.route == AGG_AUTO_ONE_LAUNCH) {
        const AutoLaunch o = old_launch_match_auto_small(f, mp, n, f.cus), &x = p.auto_launch;
        if (!extension) ++specs;
        SPEC_EQ("auto.th", x.th, o.th);
        SPEC_EQ("auto.wide", x.wide, o.wide);
        SPEC_EQ("auto.pk", x.pk, o.pk);
        SPEC_EQ("auto.nsplit", x.nsplit, o.nsplit);
        SPEC_EQ("auto.nd_chunk", x.nd_chunk, o.nd_chunk);
        SPEC_EQ("auto.lds_bytes", x.lds_bytes, o.lds_bytes);
        if (x.lds_bytes > (size_t)MATCH_AUTO_LDS_CAP) violation("one-launch LDS beyond the cap: %s", describe(c, call, n, whole));
        if ((size_t)x.nsplit * n * SMX_SLICE_WORDS * f.h * f.w > f.slices_floats) violation("one-launch records do not fit the lane's slice region: %s", describe(c, call, n, whole));
        if (x.th != 8 && x.th != 10 && x.th != 12) violation("one-launch band height: %s", describe(c, call, n, whole));
    }
    if (p.route == AGG_FILTERED) {
        const FilterLaunch o = old_launch_match_filter(f, mp, n, f.cus);
        if (!extension) ++specs;
        SPEC_EQ("filter.th", p.filter.th, o.th);
        SPEC_EQ("filter.wide", p.filter.wide, o.wide);
        SPEC_EQ("filter.pk", p.filter.pk, o.pk);
        if (p.filter.th != 24 && p.filter.th != 27 && p.filter.th != 32) violation("filter band height: %s", describe(c, call, n, whole));
    }
#undef SPEC_EQ
}

// item 5 of the head comment: the prologue (a refused plan has one too) ...
static void check_prologue(const Config &c, const EngineFacts &f, const CallFacts &call, const RangePlan &p, int n, bool whole) {
    const int W = c.w * c.K - c.crop;
    const bool u8 = call.in_mode == IN_GRAY_U8 || call.in_mode == IN_RGB_U8;
    for (int aligned = 1; aligned >= 0; --aligned) {
        CallFacts ca = call;
        ca.u8_aligned = aligned != 0;
        // (an unaligned call: the whole plan once more where the entry reads u8, the spec function alone elsewhere)
        const PrologueLaunch x = ca.u8_aligned == call.u8_aligned ? p.prologue : (u8 ? plan_range(f, ca, n, whole).prologue : prologue_launch(f, ca));
        const int o = old_launch_prologue(ca.in_mode, c, f, ca.u8_aligned);
        prologues[x.kernel]++;
        mix2(x.in_mode * 4 + x.kernel);
        if (x.in_mode != ca.in_mode || x.kernel != o) violation("spec prologue: %d, the parent's launcher %d: %s", x.kernel, o, describe(c, ca, n, whole));
        if (x.kernel == PROLOGUE_K2 && (c.K != 2 || (ca.in_mode != IN_GRAY_F32 && ca.in_mode != IN_GRAY_U8) || (W & 1))) violation("K = 2 prologue: %s", describe(c, ca, n, whole));
        if (x.kernel == PROLOGUE_K4 && (c.K != 4 || !f.grid_capable || (W & 3) || (u8 && !ca.u8_aligned))) violation("K = 4 prologue: %s", describe(c, ca, n, whole));
    }
}
// ... step 6, the fill, the gates and the parameters of the aggregation launches
static void check_rest(const Config &c, const EngineFacts &f, const CallFacts &call, const RangePlan &p, int n, bool whole) {
#define d describe(c, call, n, whole)
    // step 6: enqueue_range computed sad_exact from the configuration on every call (min_disparity = dmin * K here)
    const bool old_sad_exact = (long long)c.K * ((long long)(c.dmin * c.K) / c.K + c.Dd) <= 271;
    const RefineLaunch &r = p.refine;
    if (r.sad_exact != old_sad_exact) violation("spec refine.sad_exact: %d, enqueue_range %d: %s", r.sad_exact ? 1 : 0, old_sad_exact ? 1 : 0, d);
    if (r.sad_exact != (c.K * (c.dmin + c.Dd) <= 271)) violation("sad_exact against the bound: %s", d);
    if (r.kind != REFINE_FLOAT && (r.kt == 0 || !f.has_u8_planes() || r.apron)) violation("integer step 6 without kt or the u8 planes: %s", d);
    if (r.kt != 0 && r.kt != 1 && r.kt != 2 && r.kt != 4) violation("refine kt: %s", d);
    if (r.apron && (r.kt == 0 || !p.owns_gray)) violation("refine apron: %s", d);
    if (!r.sad_exact) ++sx0;
    // the fill: launch_fill chose from (fp.K, px), enqueue_range computed log2k
    int old_log2k = 0;
    while ((1 << old_log2k) < c.K) old_log2k++;
    const FillInst fo = old_launch_fill(c.K, call.on_lanes && n > 4 ? 4 : 8), fn = fill_inst(p.fill);
    if (fn.kernel != fo.kernel || fn.K != fo.K || fn.px != fo.px || p.fill.K != c.K || p.fill.log2k != old_log2k)
        violation("spec fill: %d %d %d log2k %d, the parent %d %d %d log2k %d: %s", fn.kernel, fn.K, fn.px, p.fill.log2k, fo.kernel, fo.K, fo.px, old_log2k, d);
    fills[p.fill.kernel]++;
    mix2(((r.sad_exact ? 1 : 0) * 4 + p.fill.kernel) * 64 + p.fill.K * 4 + p.fill.log2k);
    // the aggregation launches: what the parent's enqueue_range handed each, against the parameter functions
    RangeParams b;
    b.mp = engine_params(c, f, p, call.on_lanes);
    b.mp.Ld = b.mp.Rd = dummy_f; b.mp.wta = b.mp.costs = b.mp.slices = dummy_f;
    b.mp.flags = dummy_flags; b.mp.epoch = 7; b.mp.tickets = dummy_tickets;
    b.range_flags = dummy_flags2;
    b.fast_stats = dummy_stats;
    const OldParams o = old_enqueue_range(f, p, b.mp, n);
    auto cmp = [&](const char *what, const MatchParams &got, const MatchParams &want) {
        ++params_compared;
        if (!same_params(got, want)) violation("params %s (gate %d / %d, nsplit %d / %d, pairs %d / %d, nd_chunk %d / %d): %s", what, got.gate, want.gate,
                                               got.nsplit, want.nsplit, got.pairs, want.pairs, got.nd_chunk, want.nd_chunk, d);
        for (long long v : {(long long)got.gate, (long long)(got.flags == dummy_flags2), (long long)got.nsplit, (long long)got.pairs, (long long)got.nd_chunk,
                            (long long)(got.tickets != nullptr), (long long)got.dense, (long long)got.dense_small, (long long)(got.fast_stats != nullptr),
                            (long long)got.fast_stride, (long long)got.unit})
            mix2(v);
    };
    const bool gated = p.route == AGG_AUTO_GATED;
    if (has_exact(p)) {
        const MatchParams m = exact_params(b, p.exact, n);
        cmp("exact", m, o.exact);
        if (p.exact.split > 1 && (m.nsplit != p.exact.split || m.pairs != n || m.tickets)) violation("split launch parameters: %s", d);
        if (p.exact.gate != (p.route == AGG_FILTERED || gated ? 2 : 0) || (p.exact.gate_flag == GATE_RANGE_FLAG) != (p.route == AGG_FILTERED))
            violation("exact gate: %s", d);
    }
    if (has_exact_capture(p)) {
        cmp("exact_capture", exact_capture_params(b, p.exact_capture), o.exact_capture);
        if (p.exact_capture.gate != (gated ? 2 : 0)) violation("exact capture gate: %s", d);
    }
    if (has_fast(p)) {
        cmp("fast", fast_params(b, p, p.fast_launch.gate), o.fast);
        if (p.capture_follows) cmp("fast_capture", fast_params(b, p, p.fast_capture.gate), o.fast_capture);
        if (p.fast_launch.gate != (gated ? 1 : 0) || (p.capture_follows && p.fast_capture.gate != p.fast_launch.gate)) violation("fast gate: %s", d);
    }
    if (gated)      // both on the grid flag: exactly one of the pair does the work, whatever the flag says
        for (int flag = 0; flag < 2; ++flag)
            if (p.exact.gate_flag != GATE_GRID_FLAG || gate_runs(p.exact.gate, flag != 0) == gate_runs(p.fast_launch.gate, flag != 0) ||
                (p.capture_follows && gate_runs(p.exact_capture.gate, flag != 0) == gate_runs(p.fast_capture.gate, flag != 0)) ||
                (p.capture_follows && gate_runs(p.exact_capture.gate, flag != 0) != gate_runs(p.exact.gate, flag != 0)))
                violation("gated pair: %s", d);
    if (p.route == AGG_AUTO_ONE_LAUNCH) cmp("auto", auto_params(b, p, n), o.auto_small);
    if (p.route == AGG_FILTERED) {
        cmp("filter", filter_params(b, f), o.filter);
        cmp("sparse", sparse_params(b, f), o.sparse);
    }
#undef d
}

static void check_plan(const Config &c, const EngineFacts &f, const CallFacts &call, int n, bool whole) {
    const RangePlan p = plan_range(f, call, n, whole);
    if (reach_keys) {
        if (p.status == SMX_OK) keys_of(p, *reach_keys);
        return;
    }
    check_prologue(c, f, call, p, n, whole);
    if (extension) {
        if (p.status == SMX_OK) {
            check_specs(c, f, call, p, n, whole);
            check_rest(c, f, call, p, n, whole);
        }
        return;
    }
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
    refines[p.refine.kind]++;
    // every field enqueue_range reads, one per bit field (the stride as the launch gets it: only with a report)
    unsigned long long word = 0;
    for (unsigned v : {(unsigned)p.mode, (unsigned)p.route, (unsigned)p.gated_dense_first, (unsigned)p.exact_split, (unsigned)p.capture_follows,
                       (unsigned)p.fast.small, (unsigned)p.fast.th, (unsigned)p.fast.wide, (unsigned)p.dense, (unsigned)p.dense_small, (unsigned)p.reports,
                       (unsigned)(p.fill_publishes ? p.stride : 0), (unsigned)p.fill_publishes, (unsigned)p.owns_gray, (unsigned)p.refine.kind,
                       (unsigned)p.refine.kt, (unsigned)p.refine.apron, (unsigned)p.refine_reports_grid, (unsigned)p.fill.px})
        word = word * 67 + v;
    mix((long long)word);
    // ... and every field of the launch specs (value-initialised where the route has no such launch)
    unsigned long long sw = 0;
    for (long long v : {(long long)p.exact.kernel, (long long)p.exact.split, (long long)p.exact.rows_per_thread, (long long)p.exact.nd_chunk,
                        (long long)p.exact.lds_bytes, (long long)p.exact.slice_floats, (long long)p.exact_capture.split,
                        (long long)p.exact_capture.rows_per_thread, (long long)p.exact_capture.nd_chunk, (long long)p.exact_capture.lds_bytes,
                        (long long)p.fast_launch.th, (long long)p.fast_launch.small, (long long)p.fast_launch.pitch, (long long)p.fast_launch.pk,
                        (long long)p.fast_launch.argb, (long long)p.fast_launch.form, (long long)p.fast_capture.small, (long long)p.fast_capture.wide,
                        (long long)p.fast_capture.pk, (long long)p.auto_launch.th, (long long)p.auto_launch.wide, (long long)p.auto_launch.pk,
                        (long long)p.auto_launch.nsplit, (long long)p.auto_launch.nd_chunk, (long long)p.auto_launch.lds_bytes,
                        (long long)p.filter.th, (long long)p.filter.wide, (long long)p.filter.pk})
        sw = sw * 1000003ull + (unsigned long long)v;
    mix((long long)sw);
    check_specs(c, f, call, p, n, whole);
    check_rest(c, f, call, p, n, whole);
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
    if (p.fill.px != (call.on_lanes && n > 4 ? 4 : 8)) violation("fill width: %s", describe(c, call, n, whole));
    if (p.refine_reports_grid && (p.refine.kind != REFINE_AUTO || !whole)) violation("grid report: %s", describe(c, call, n, whole));
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
    if (!reach_keys && (f.capture != (c.default_radii && c.dmin > 0 && c.dmin <= c.Dd) || f.has_volume != (c.dmin > 0 && !f.capture) || (f.filter_ok && f.has_volume)))
        violation("facts: %s", describe(c, CallFacts{}, 0, false));
    for (int in_mode : {IN_GRAY_F32, IN_RGB_F32, IN_GRAY_U8, IN_RGB_U8})
        for (int on_lanes = 0; on_lanes < 2; ++on_lanes)
            for (int n = 1; n <= c.B; ++n) {
                if (!reach_keys && !extension) check_kind(c, f, in_mode, on_lanes != 0, n, 0);
                if (!reach_keys && !extension && on_lanes && n >= 2) check_kind(c, f, in_mode, true, (n + 1) / 2, n - (n + 1) / 2);
                CallFacts call;
                call.in_mode = in_mode;
                call.on_lanes = on_lanes != 0;
                for (int whole = 0; whole < 2; ++whole)
                    for (int dense = 0; dense < 2; ++dense)
                        for (int filt = 0; filt < 2; ++filt)
                            for (int hint = -1; hint <= 1; ++hint) {
                                // (`reach`: only k_refine_auto reports the grid flag; an engine without the u8 planes never holds a hint)
                                if (reach_keys && hint != -1 && (f.kt == 0 || !f.has_u8_planes())) continue;
                                call.route.fast_dense = dense != 0;
                                call.route.use_filter = filt != 0;
                                call.route.grid_hint = hint;
                                check_plan(c, f, call, n, whole != 0);
                            }
            }
}

// only_cus > 0 (`reach`): the same configurations on that CU count alone, at the two smallest shapes (large: the other two)
static void sweep(int only_cus = 0, bool large = false) {
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
                                            if (only_cus > 0 && (cus != 256 || (shape[0] > 64) != large)) continue;
                                            Config c;
                                            c.default_radii = radii == 0; c.K = K; c.dmin = dmin; c.h = shape[0]; c.w = shape[1]; c.Dd = Dd;
                                            c.B = B; c.match_mode = mode; c.cus = only_cus > 0 ? only_cus : cus; c.sad = sad;
                                            c.opt.fast_dense = opt[0]; c.opt.fast_dense_small = opt[1];
                                            c.exact_filter = cus == 80 ? 1 : (defaults && sad == 5 ? 0 : -1);     // all three values
                                            sweep_facts(c);
                                        }
}

// The extension of item 5: what the sweep above does not hold and the specs of item 5 depend on -- K = 8 (the power-of-two
// generic fill, kt = 0) and widths that are no multiple of K (the prologue's fallbacks) -- in AUTO mode on 256 CUs.
static void sweep_extension(int only_cus = 0, bool large = false) {
    const int shapes[3][2] = {{48, 80}, {64, 128}, {187, 621}};
    const int kc[6][2] = {{8, 0}, {8, 4}, {2, 1}, {3, 1}, {4, 1}, {4, 2}};
    extension = true;
    for (const auto &k : kc)
        for (int dmin : {0, 8})
            for (const auto &shape : shapes)
                for (int Dd : {16, 64})
                    for (int B : {1, 4, 64}) {
                        if (only_cus > 0 && (shape[0] > 64) != large) continue;
                        Config c;
                        c.K = k[0]; c.crop = k[1]; c.dmin = dmin; c.h = shape[0]; c.w = shape[1]; c.Dd = Dd; c.B = B;
                        c.cus = only_cus > 0 ? only_cus : 256;
                        sweep_facts(c);
                    }
    extension = false;
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
        expect(p.refine.kind == REFINE_FLOAT && p.refine.kt == 2 && p.refine.apron && p.owns_gray, "refine RGB: float, on the engine's aproned planes");
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 4, wc);
        expect(p.refine.kind == REFINE_INT && p.refine.kt == 2 && !p.refine.apron, "refine u8 gray n=4: int");
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 5, wc);
        expect(p.refine.kind == REFINE_INT_V, "refine u8 gray n=5: int_v");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, -1), 4, wc);
        expect(p.refine.kind == REFINE_AUTO && p.refine_reports_grid == wc && !p.owns_gray, "refine f32 gray n=4: auto, reports the grid flag iff whole call");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, -1), 5, wc);
        expect(p.refine.kind == REFINE_AUTO_V && !p.refine_reports_grid, "refine f32 gray n=5: auto_v");
        // fill width
        for (int n : {4, 5, 32})
            for (int lanes = 0; lanes < 2; ++lanes) {
                p = plan_range(f, call_of(IN_GRAY_U8, lanes != 0, false, true, -1), n, wc);
                expect(p.fill.px == (lanes && n > 4 ? 4 : 8), "fill width: 4 iff on the lanes and n > 4");
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
        expect(p.status == SMX_OK && p.route == AGG_EXACT && p.refine.kind == REFINE_FLOAT && p.refine.kt == 0, "K = 3, AUTO: exact, generic step 6");
    }
    {   // sad_patch_radius 4: the generic float step-6 kernel, whatever the entry
        Config c = c2;
        c.sad = 4;
        const EngineFacts f4 = facts_of(c);
        for (int in_mode : {IN_GRAY_F32, IN_RGB_F32, IN_GRAY_U8, IN_RGB_U8}) {
            const RangePlan p = plan_range(f4, call_of(in_mode, false, false, true, -1), 4, true);
            expect(p.refine.kind == REFINE_FLOAT && p.refine.kt == 0 && !p.refine.apron && !p.refine_reports_grid, "sad_patch_radius 4: float, kt 0");
        }
    }
    {   // the launch specs of the examples the source comments give (k_match_exact2.h: exact_split, capture_split; tu_fast_small.hip)
        RangePlan p = plan_range(f, call_of(IN_RGB_U8, false, false, true, -1), 1, true);
        expect(f.e2_tiles == 60 && p.route == AGG_EXACT && p.exact.kernel == EXACT_TILED && p.exact.split == 8 && p.exact.nd_chunk == 8 &&
               p.exact.rows_per_thread == 2 && p.exact.slice_floats == (size_t)8 * SMX_SLICE_WORDS * 188 * 621, "C2 pair: 60 tiles, 8 slices of 8");
        p = plan_range(f, call_of(IN_RGB_U8, false, false, true, -1), 1, false);
        expect(p.exact.split == 1 && p.exact.rows_per_thread == 4 && p.exact.nd_chunk == f.exact2_nd && p.exact.slice_floats == 0, "C2 pair as a half: unsplit");
        Config c = c2;                                          // the reference's default configuration: 1080p, K 2, disparities 75 .. 262
        c.h = 540; c.w = 960; c.dmin = 37; c.Dd = 95; c.B = 1;
        const EngineFacts fd = facts_of(c);
        p = plan_range(fd, call_of(IN_RGB_U8, false, false, true, -1), 1, true);
        expect(fd.e2_tiles == 272 && fd.capture && p.route == AGG_EXACT && p.exact.split == 7 && p.exact.nd_chunk == 14 && p.capture_follows &&
               p.exact_capture.split == 3 && p.exact_capture.rows_per_thread == 2, "1080p default: 272 tiles x 95 disparities, 7 slices of 14, capture split 3");
        c = c2;                                                  // 64 pooled rows: the sparse plan's bands are 32 rows high
        c.h = 64; c.w = 128; c.B = 256; c.Dd = 256;
        EngineFacts fb = facts_of(c);
        p = plan_range(fb, call_of(IN_GRAY_U8, false, true, true, -1), 200, true);
        expect(p.route == AGG_FAST && !p.fast.small && p.fast.th == 32 && p.dense && p.fast_launch.th == 27 && p.fast_launch.form == FAST_DENSE &&
               p.fast_launch.argb && p.fast_launch.pitch == 320, "32-row plan, dense form, Dd 256: launches 27 rows");
        p = plan_range(fb, call_of(IN_GRAY_U8, false, false, true, -1), 200, true);
        expect(p.fast.th == 32 && p.fast_launch.th == 32 && p.fast_launch.form == FAST_SPARSE, "32-row plan, sparse form: launches 32 rows");
        c.Dd = 257;
        fb = facts_of(c);
        p = plan_range(fb, call_of(IN_GRAY_U8, false, true, true, -1), 200, true);
        expect(p.fast.th == 32 && p.dense && p.fast_launch.th == 32 && p.fast_launch.form == FAST_SPARSE && !p.fast_launch.argb,
               "32-row plan, dense form, Dd 257: launches 32 rows sparse (no dense instantiation)");
    }
    {   // the specs around the aggregation: steps 1-2 ...
        auto prologue = [](int K, int w, int crop, int in_mode, bool aligned) {
            Config c;
            c.K = K; c.h = 48; c.w = w; c.crop = crop; c.Dd = 16;
            CallFacts call = call_of(in_mode, false, false, true, -1);
            call.u8_aligned = aligned;
            const RangePlan p = plan_range(facts_of(c), call, 1, true);
            return p.prologue.in_mode == in_mode ? p.prologue.kernel : -1;
        };
        expect(prologue(2, 80, 0, IN_GRAY_F32, true) == PROLOGUE_K2 && prologue(2, 80, 0, IN_GRAY_U8, false) == PROLOGUE_K2, "K = 2, W = 160, gray: two pixels per thread, whatever the alignment");
        expect(prologue(2, 80, 1, IN_GRAY_F32, true) == PROLOGUE_GENERIC && prologue(2, 80, 1, IN_GRAY_U8, true) == PROLOGUE_GENERIC, "K = 2, W = 159 (odd): generic");
        expect(prologue(2, 80, 0, IN_RGB_F32, true) == PROLOGUE_GENERIC && prologue(2, 80, 0, IN_RGB_U8, true) == PROLOGUE_GENERIC, "K = 2, RGB: generic");
        for (int in_mode : {IN_GRAY_F32, IN_RGB_F32, IN_GRAY_U8, IN_RGB_U8}) {
            const bool u8 = in_mode == IN_GRAY_U8 || in_mode == IN_RGB_U8;
            expect(prologue(4, 80, 0, in_mode, true) == PROLOGUE_K4, "K = 4, W = 320: the block kernel");
            expect(prologue(4, 80, 2, in_mode, true) == PROLOGUE_GENERIC, "K = 4, W = 318: generic");
            expect(prologue(4, 80, 0, in_mode, false) == (u8 ? PROLOGUE_GENERIC : PROLOGUE_K4), "K = 4, W = 320, pointers off by a byte: generic for the u8 entries only");
            expect(prologue(1, 80, 0, in_mode, true) == PROLOGUE_GENERIC && prologue(3, 80, 0, in_mode, true) == PROLOGUE_GENERIC &&
                   prologue(8, 80, 0, in_mode, true) == PROLOGUE_GENERIC, "K = 1, 3, 8: generic");
        }
        Config c = c2;
        c.match_mode = SMX_MATCH_FAST_GRID;
        c.K = 3;
        expect(plan_range(facts_of(c), call_of(IN_RGB_U8, false, false, true, -1), 1, true).prologue.in_mode == IN_RGB_U8, "a refused plan names its prologue");
    }
    {   // ... step 6: the SAD parabola is exact up to |abscissa| 271 = K * (min_disparity / K + disparities) ...
        Config c;
        c.h = 32; c.w = 160; c.Dd = 135;                        // max_disparity 269: 2 * 135 = 270
        EngineFacts fs = facts_of(c);
        expect(fs.sad_exact && fs.has_u8_planes() && plan_range(fs, call_of(IN_GRAY_U8, false, false, true, -1), 1, true).refine.sad_exact, "K 2, 135 disparities: exact");
        c.Dd = 136;                                             // max_disparity 271: 2 * 136 = 272, left apron 284 of 320 columns
        fs = facts_of(c);
        expect(!fs.sad_exact && fs.has_u8_planes() && fs.padl == 284, "K 2, 136 disparities: beyond the bound, u8 planes fit");
        const int kinds[4][3] = {{IN_GRAY_U8, 1, REFINE_INT}, {IN_GRAY_U8, 5, REFINE_INT_V}, {IN_GRAY_F32, 1, REFINE_AUTO}, {IN_GRAY_F32, 5, REFINE_AUTO_V}};
        for (const auto &k : kinds) {
            const RangePlan p = plan_range(fs, call_of(k[0], false, false, true, -1), k[1], true);
            expect(p.refine.kind == k[2] && p.refine.kt == 2 && !p.refine.sad_exact && !p.refine.apron, "136 disparities: the evaluating integer kernels");
        }
        c.Dd = 128; c.dmin = 8;                                 // min_disparity counts: 2 * (8 + 128) = 272
        expect(!facts_of(c).sad_exact, "min_disparity 16, 128 disparities: beyond the bound");
        c = c2;
        c.K = 8;
        const RangePlan p = plan_range(facts_of(c), call_of(IN_GRAY_U8, false, false, true, -1), 1, true);
        expect(p.refine.kind == REFINE_FLOAT && p.refine.kt == 0 && !p.refine.apron, "K = 8: generic float step 6");
    }
    {   // ... steps 7-9 ...
        const int rows[5][4] = {{1, FILL_4, 0, 4}, {2, FILL_4, 1, 8}, {3, FILL_GENERIC, 2, 0}, {4, FILL_4, 2, 8}, {8, FILL_POW2, 3, 0}};   // K, kernel, log2k, px on a caller's stream
        for (const auto &r : rows) {
            Config c = c2;
            c.K = r[0];
            const EngineFacts fk = facts_of(c);
            RangePlan p = plan_range(fk, call_of(IN_GRAY_U8, false, false, true, -1), 5, true);
            FillInst fi = fill_inst(p.fill);
            expect(p.fill.kernel == r[1] && p.fill.K == r[0] && p.fill.log2k == r[2] && fi.px == r[3], "fill kernel, log2k and pixels per thread by K");
            p = plan_range(fk, call_of(IN_GRAY_U8, true, false, true, -1), 5, true);
            fi = fill_inst(p.fill);
            expect(fi.px == (r[0] == 2 || r[0] == 4 ? 4 : r[3]), "on the lanes, 5 pairs: 4 pixels per thread at K = 2 / 4");
        }
    }
    {   // ... the gates and the parameters of a split launch
        RangePlan p = plan_range(f, call_of(IN_RGB_F32, false, false, true, -1), 32, true);
        expect(p.route == AGG_FILTERED && p.exact.gate == 2 && p.exact.gate_flag == GATE_RANGE_FLAG && p.exact.split == 1, "filtered, f32 RGB: the dense launch runs for flagged pairs, on the range flag");
        p = plan_range(f, call_of(IN_GRAY_F32, false, false, true, 1), 1, true);
        expect(p.route == AGG_AUTO_GATED && p.exact.gate == 2 && p.exact.gate_flag == GATE_GRID_FLAG && p.fast_launch.gate == 1, "gated: exact-order 2, fast 1, on the grid flag");
        RangeParams b;
        b.mp.tickets = dummy_tickets; b.mp.flags = dummy_flags; b.range_flags = dummy_flags2;
        MatchParams m = exact_params(b, p.exact, 1);
        expect(p.exact.split == 8 && m.gate == 2 && m.nsplit == 8 && m.pairs == 1 && m.nd_chunk == 8 && !m.tickets && m.flags == dummy_flags, "gated split launch: 8 slices, records of 1 pair, no tickets");
        m = fast_params(b, p, p.fast_launch.gate);
        expect(m.gate == 1 && m.nsplit == 0 && m.tickets == dummy_tickets, "gated fast launch: gate 1");
        p = plan_range(f, call_of(IN_GRAY_U8, false, false, true, -1), 1, true);
        expect(p.route == AGG_FAST && p.fast_launch.gate == 0 && p.exact.gate == 0, "u8 gray: ungated");
        Config c = c2;
        c.dmin = 8;
        p = plan_range(facts_of(c), call_of(IN_GRAY_F32, false, false, true, 1), 1, true);
        expect(p.capture_follows && p.exact_capture.gate == 2 && p.fast_capture.gate == 1, "capture, gated: the lookups carry their arg-max launch's gate");
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

static void print_keys(const char *head, const std::set<std::string> &keys) {
    printf("%s", head);
    for (const std::string &k : keys) printf(" %s", k.c_str());
    printf("\n");
}

int main(int argc, char **argv) {
    if (argc == 3 && !strcmp(argv[1], "reach")) {
        std::set<std::string> small, large, only;
        reach_keys = &small;
        sweep(atoi(argv[2]), false);
        sweep_extension(atoi(argv[2]), false);
        reach_keys = &large;
        sweep(atoi(argv[2]), true);
        sweep_extension(atoi(argv[2]), true);
        for (const std::string &k : large)
            if (!small.count(k)) only.insert(k);
        print_keys("reach-small", small);
        print_keys("reach-large-only", only);
        return 0;
    }
    if (argc == 22 && !strcmp(argv[1], "spec")) {
        int a[20];
        for (int i = 0; i < 20; ++i) a[i] = atoi(argv[2 + i]);
        Config c;
        c.cus = a[0]; c.default_radii = a[1] != 0; c.K = a[2]; c.h = a[3]; c.w = a[4]; c.Dd = a[5]; c.dmin = a[6]; c.B = a[7]; c.match_mode = a[8];
        c.opt.fast_dense = a[9]; c.opt.fast_dense_small = a[10]; c.crop = a[18];
        CallFacts call = call_of(a[11], a[12] != 0, a[13] != 0, a[14] != 0, a[15]);
        call.u8_aligned = a[19] != 0;
        const RangePlan p = plan_range(facts_of(c), call, a[16], a[17] != 0);
        std::set<std::string> keys;
        if (p.status == SMX_OK) keys_of(p, keys);
        print_keys("keys", keys);
        return p.status == SMX_OK ? 0 : 2;
    }
    directed_table();
    sweep();
    sweep_extension();
    printf("launch-plan plans %ld kinds %ld directed %ld routes %ld %ld %ld %ld %ld refused %ld refine %ld %ld %ld %ld %ld hash %016llx violations %ld "
           "specs %ld exact %ld %ld %ld split %ld form %ld %ld %ld %ld dense-fallback %ld hash2 %016llx prologue %ld %ld %ld fill %ld %ld %ld sx0 %ld params %ld\n",
           plans, kinds, directed, routes[AGG_FILTERED], routes[AGG_EXACT], routes[AGG_FAST], routes[AGG_AUTO_ONE_LAUNCH], routes[AGG_AUTO_GATED],
           refused, refines[REFINE_FLOAT], refines[REFINE_INT], refines[REFINE_INT_V], refines[REFINE_AUTO], refines[REFINE_AUTO_V], plan_hash, violations,
           specs, exact_kernels[EXACT_GENERIC], exact_kernels[EXACT_GENERIC_VOLUME], exact_kernels[EXACT_TILED], exact_splits, forms[FAST_SPARSE],
           forms[FAST_PASS1_ONLY], forms[FAST_DENSE], forms[FAST_DENSE_SMALL], dense_fallbacks, plan_hash2, prologues[PROLOGUE_GENERIC], prologues[PROLOGUE_K2],
           prologues[PROLOGUE_K4], fills[FILL_4], fills[FILL_POW2], fills[FILL_GENERIC], sx0, params_compared);
    return violations == 0 ? 0 : 1;
}
