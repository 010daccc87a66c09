// smx_plan.h -- the one place where a call's launches are decided.
//
// derive_facts() turns a configuration into everything the plans depend on that is fixed after smx_create; plan_range()
// turns those facts, the call (entry, stream lanes or caller's stream, the decision of the content switches) and a range
// of n pairs into a RangePlan: the prologue, the aggregation kernels and their form, the step-6 and the fill launch.
// Every launch of the range is named by a launch spec (smx_common.h): PrologueLaunch (entry; generic, K = 2 two-pixel or
// K = 4 block kernel), the aggregation family (ExactLaunch, ExactCaptureLaunch, FastLaunch, FastCaptureLaunch, AutoLaunch,
// FilterLaunch: the kernel instantiation -- band height as launched, pitch, packed-sum form, form of the fast kernel,
// disparity split, rows per thread -- with its right-tile chunk, dynamic LDS, slice records and its gate), RefineLaunch
// (kernel, compile-time K, aprons, exact SAD parabola) and FillLaunch (kernel, pixels per thread).  The parameter functions
// at the end of this header (exact_params, ..., auto_params) turn the parameters a range's launches share and a spec into
// that launch's MatchParams.  The launchers behind smx_launch.h are tables from spec to instantiation; nothing below this
// header decides anything.  smx_engine.hip executes the plan (enqueue_range binds the buffers and walks the route),
// predicts from it which content switch a call can report to (call_kind) and answers its queries from it; the CPU
// harnesses under tests/ compile the same lines, so what a call launches, and with which parameters, can be read, and
// swept, without a GPU.
//
// Host-only inline functions without a HIP runtime call, like smx_route.h; the kernel headers are included for their
// constants and for the helpers that hold the tuning (match_fast_plan, exact_split, capture_split, match_auto_nsplit,
// filter_plan, fast_tall_pitch, match_auto_small_applicable, ...).
#pragma once

#include "../../include/stereo_mi355x.h"
#include "k_match_auto.h"
#include "k_match_capture.h"
#include "k_match_exact.h"
#include "k_match_exact2.h"
#include "k_match_fast.h"
#include "k_match_filter.h"
#include "k_prologue.h"
#include "smx_common.h"
#include "smx_launch.h"
#include "smx_route.h"

namespace smx {

// Dynamic LDS the register-tiled exact-order kernels size their right-tile chunk against (two workgroups per CU).
constexpr int SMX_EXACT2_LDS_CAP = 80 * 1024;

// Environment switches that force a form of the fast kernel (tests, A/B runs): 1 / 0: always / never, -1: by content.
struct PlanOptions {
    int fast_dense = -1;            // SMX_FAST_DENSE
    int fast_dense_small = -1;      // SMX_FAST_DENSE_SMALL: the latency shape at 12-row bands
    int fast_stack = -1;            // SMX_FAST_STACK: the stacked bands of the throughput shape (-1: on the stream lanes, where they march fewer rows)
};

// Everything the launch plans depend on that is fixed after smx_create.
struct EngineFacts {
    // configuration
    int match_mode = SMX_MATCH_AUTO, exact_filter = 0;
    int B = 1, h = 0, w = 0, dmin = 0, Dd = 0, K = 1;
    int sad_patch_radius = 5;
    int cus = 256;                  // multiProcessorCount of the device: launch plans are sized against it
    PlanOptions opt;
    // derived
    bool grid_capable = false;      // K in {1,2,4,8}: 1/K^2 grid sums are exact
    bool default_radii = false;     // ncc 1, block-matching radii 1 / 4 / 10
    bool fast_ok = false;           // K and radii admit the FAST_GRID kernel
    bool filter_ok = false;         // the configuration admits the filtered route (k_match_filter.h)
    bool capture = false;           // dmin > 0 served by the sparse capture kernels (no aggregated volume)
    bool has_volume = false;        // dmin > 0 otherwise: the generic exact-order kernel materialises the aggregated volume
    int kt = 0;                     // compile-time K of the specialised step-6 kernels (1, 2, 4) or 0: the generic float kernel
    int pitch8 = 0, padl = 0, padr = 0;   // u8 planes with cyclic aprons; pitch8 = 0: integer step-6 kernel not applicable
    int gpitch = 0, gpadl = 0;            // row pitch / left-apron width (floats) of the engine's gray planes
    int upitch = 0;                       // row pitch (u16) of the pooled planes in grid units (smx_common.h: unit_plane_pitch)
    bool prologue_k2 = false;       // K = 2, even W: the gray entries pool two pixels per thread with 16-byte loads
    bool prologue_k4 = false;       // K = 4, W a multiple of 4 and so is every pitch and apron: one pooled pixel is a 4 x 4 block of 16-byte loads
    bool sad_exact = true;          // step 6, integer kernels: the SAD parabola is exact for every disparity (k_refine.h refine_finish_int)
    int exact_nd = 0, exact2_nd = 0;      // disparities per right-tile load: generic / register-tiled exact-order kernel
    size_t exact_lds = 0, exact2_lds = 0;
    int e2_tiles = 0;               // exact-order tiles per pair: arrival tickets of the one-launch AUTO kernel (default radii)
    size_t slices_floats = 0;       // one stream lane's region of the slice buffer (0: none)
    int cand_tiles_x = 0, cand_tiles_y = 0, cand_cw = 0;   // candidate bits of the filtered route
    int filter_unit = 0;            // grid units per gray level of the filter's rounded inputs (>= K^2)
    float filter_two_e = 0.f;       // twice the filter's error bound, in aggregation units
    // the report words of the two content switches exist (device counters and the pinned hint words)
    bool filter_words = false, fast_words = false;

    bool has_u8_planes() const { return pitch8 != 0; }
    bool has_tickets() const { return default_radii; }
    bool has_slices() const { return slices_floats != 0; }
};

// LDS bytes of the generic exact-order kernel's tile at the largest right-tile chunk (*nd disparities) that keeps it within
// 64 KB; more than 64 KB even at one disparity: the radii are not supported (smx_create refuses).
inline size_t exact_tile_lds(const smx_config &cfg, int Dd, int *nd) {
    *nd = Dd;
    while (*nd > 1 && exact_lds_floats((int)cfg.ncc_patch_radius, cfg.large_mbm_radius, *nd) * sizeof(float) > 64 * 1024)
        *nd = (*nd + 1) / 2;
    return exact_lds_floats((int)cfg.ncc_patch_radius, cfg.large_mbm_radius, *nd) * sizeof(float);
}

inline EngineFacts derive_facts(const smx_config &cfg, const smx_dims &d, int cus, PlanOptions opt) {
    EngineFacts f;
    f.match_mode = cfg.match_mode; f.exact_filter = cfg.exact_filter;
    f.B = cfg.max_batch > 0 ? cfg.max_batch : 1;
    f.h = d.h; f.w = d.w; f.dmin = d.dmin; f.Dd = d.Dd; f.K = d.K;
    f.sad_patch_radius = (int)cfg.sad_patch_radius;
    f.cus = cus;
    f.opt = opt;
    const int K = d.K;
    f.grid_capable = (K == 1 || K == 2 || K == 4 || K == 8);
    f.default_radii = cfg.ncc_patch_radius == 1 && cfg.small_mbm_radius == 1 && cfg.mid_mbm_radius == 4 &&
                      cfg.large_mbm_radius == 10;
    f.fast_ok = f.grid_capable && f.default_radii;
    f.exact_lds = exact_tile_lds(cfg, d.Dd, &f.exact_nd);
    // register-tiled exact kernel: up to 80 KB of LDS (two workgroups per CU), opt-in above 64 KB
    int nd2 = d.Dd;
    while (nd2 > 1 && exact2_lds_floats(nd2) * sizeof(float) > (size_t)SMX_EXACT2_LDS_CAP) nd2 = (nd2 + 1) / 2;
    f.exact2_nd = nd2;
    f.exact2_lds = exact2_lds_floats(nd2) * sizeof(float);
    {   // cyclic column aprons wide enough for every shifted step-6 window (u8 planes and float gray alike)
        const int padl = (8 + K * (d.dmax + 2) + 3) & ~3, padr = (32 + K + 3) & ~3;
        f.kt = (cfg.sad_patch_radius == 5 && (K == 1 || K == 2 || K == 4)) ? K : 0;
        if (f.kt != 0 && padl <= d.W && padr <= d.W) {
            f.padl = padl; f.padr = padr;
            f.pitch8 = (padl + d.W + padr + 3) & ~3;
            f.gpitch = f.pitch8;
            f.gpadl = padl;
        } else {
            f.gpitch = d.W;
            f.gpadl = 0;
        }
    }
    f.upitch = unit_plane_pitch(d.w);
    f.prologue_k2 = K == 2 && (d.W & 1) == 0;
    f.prologue_k4 = K == 4 && (d.W & 3) == 0 && f.grid_capable && (f.gpitch & 3) == 0 && (f.gpadl & 3) == 0 && (f.pitch8 & 3) == 0 &&
                    (f.padl & 3) == 0 && (f.gpadl == 0 || f.gpadl == f.padl);
    // largest |abscissa| of the SAD parabola: d_hi = K * (dmin / K + Dd) (k_refine.h refine_finish_int: exact up to 271)
    f.sad_exact = (long long)K * ((long long)cfg.min_disparity / K + d.Dd) <= 271;
    if (f.default_radii) {
        // slice records of the disparity-split exact kernel and of the one-launch AUTO kernel's off-grid branch (few pairs
        // in flight): one region per stream lane, sized by the rule the launches check against (k_match_auto.h); arrival
        // tickets per (pair slot, tile): the last slice of a tile merges it inside the split launch
        MatchParams sp{};
        sp.h = d.h; sp.w = d.w; sp.Dd = d.Dd;
        f.slices_floats = slice_region_floats(sp, f.B, cus, f.fast_ok);
        f.e2_tiles = ((d.w + E2_TW - 1) / E2_TW) * ((d.h + E2_TH - 1) / E2_TH);
    }
    // dmin > 0: step 6 indexes the aggregated volume by absolute disparity (Q5 / rule S6).  With the default
    // radii the sparse capture kernels deliver exactly those entries; only other radii still materialise it.
    f.capture = capture_applicable(d.dmin, d.Dd) && f.default_radii;
    f.has_volume = d.dmin > 0 && !f.capture;
    // filtered exact-order route for off-grid input (gray from RGB): dmin == 0 or the capture route.  Its error bound
    // (k_match_filter.h: filter_error_bound_units) is derived for exactly these radii -- 63 / 63 / 81 taps of a 3x3
    // cost -- and for grid units up to 64 (exact integer sums below 2^24): anything else takes the dense kernel, and so
    // does the volume route, which needs every disparity anyway.
    static_assert(FILTER_TILE_H == E2_TH && FILTER_TILE_W == E2_TW, "the filter marks exact-order tiles");
    f.filter_ok = cfg.exact_filter >= 0 && f.fast_ok && f.default_radii && K * K <= 64 &&
                  filter_cand_words(d.Dd) <= E2_SPARSE_WORDS && !f.has_volume;
    if (f.filter_ok) {
        f.cand_tiles_x = (d.w + E2_TW - 1) / E2_TW;
        f.cand_tiles_y = (d.h + E2_TH - 1) / E2_TH;
        f.cand_cw = filter_cand_words(d.Dd);
        // grid unit of the filter's rounded inputs: K^2, the pooled grid.  (Measured: a finer grid -- 16 or 64 units at
        // K = 2, i.e. an error bound 3.5x / 8x smaller -- takes the candidate density of the reference's real pair from
        // 0.65 to 0.57 / 0.55 only: the flat cost curves of a real scene are genuinely ambiguous, and the filter
        // loses the packed u16 stages; profiles/r03_filter_unit.txt.)
        f.filter_unit = K * K;
        f.filter_two_e = (float)(2.0 * filter_error_bound_units((double)f.filter_unit) * (1.0 + 1e-6));
    }
    f.filter_words = f.filter_ok;       // (smx_create allocates what the facts name)
    f.fast_words = true;
    return f;
}

// One call: its entry, where it runs and what RouteState::decide_call decided for it (both halves of a split call alike).
struct CallFacts {
    int in_mode = IN_GRAY_F32;
    bool on_lanes = false;          // the call runs on the stream lanes
    bool u8_aligned = true;         // u8 entries: the caller's left | right are 4-byte aligned (the prologue's one per-call input)
    CallRoute route{false, true, -1};
};

enum AggRoute {
    AGG_FILTERED = 0,       // [gated dense exact-order,] filter, sparse exact-order [, capture]
    AGG_EXACT,              // exact-order [, capture]
    AGG_FAST,               // fast [, capture]
    AGG_AUTO_ONE_LAUNCH,    // the one-launch AUTO kernel (k_match_auto.h)
    AGG_AUTO_GATED,         // gated exact-order [, capture], gated fast [, capture]: the device-side grid flag lets one do the work
    AGG_ROUTES
};

// Everything enqueue_range does for one range of n pairs.
struct RangePlan {
    int status = SMX_OK;            // SMX_ERR_UNSUPPORTED: refused after the prologue (`refusal` says why): of the fields below only owns_gray and prologue apply
    const char *refusal = nullptr;
    int mode = SMX_MATCH_EXACT_ORDER;   // what smx_last_match_mode reports
    AggRoute route = AGG_EXACT;
    bool gated_dense_first = false; // FILTERED, f32 RGB: pairs whose gray leaves [0, 255] take the dense kernel, enqueued first
    bool exact_split = false;       // the dense exact-order launch (and its capture launch) may split the disparity range
    bool capture_follows = false;   // dmin > 0: every arg-max launch is followed by its sparse lookup launch
    bool writes_units = false;      // the prologue writes the pooled planes in grid units: some launch of the range stages from them
    FastPlan fast{};                // shape of a sparse fast-kernel launch of these n pairs (what smx_get_match_geometry reports; launched: fast_launch)
    // form of the fast kernel, on the routes that launch it (k_match_fast.h DENSE: the pass that keeps the winner's neighbours
    // instead of fetching them in a sparse second pass; min_disparity = 0 only).  Both shapes that have a dense form follow
    // the same per-call decision: the throughput shape (batches) and the latency shape at 12-row bands (single frames).
    bool dense = false, dense_small = false;
    bool reports = false;           // the sparse form samples the launch and publishes hints->fast_density ...
    int stride = 0;                 // ... of every stride-th pair
    bool fill_publishes = false;    // the fast launch of this range reports: its fill launch publishes
    // steps 6 and 7-9
    bool owns_gray = true;          // steps 6-9 read the engine's gray planes (false: the caller's, f32 gray entry)
    bool refine_reports_grid = false;   // k_refine_auto publishes the grid flag of pair 0 (hints->grid)
    // The launches of the range, as the launchers get them: steps 1-2, 6 and 7-9 ...
    PrologueLaunch prologue{};
    RefineLaunch refine{};
    FillLaunch fill{};
    // ... and the aggregation launches of the route (value-initialised where the route has no such launch):
    ExactLaunch exact{};            // FILTERED (the gated dense launch), EXACT, AUTO_GATED
    ExactCaptureLaunch exact_capture{};   // ... followed by this when capture_follows
    FastLaunch fast_launch{};       // FAST, AUTO_GATED
    FastCaptureLaunch fast_capture{};     // ... followed by this when capture_follows
    AutoLaunch auto_launch{};       // AUTO_ONE_LAUNCH
    FilterLaunch filter{};          // FILTERED

    bool has_fast_launch() const { return route == AGG_FAST || route == AGG_AUTO_ONE_LAUNCH || route == AGG_AUTO_GATED; }
};

inline bool is_rgb(int in_mode) { return in_mode == IN_RGB_F32 || in_mode == IN_RGB_U8; }

// The plan-relevant fields of a range's aggregation launches (enqueue_range fills in the buffers).
inline MatchParams plan_params(const EngineFacts &f, bool on_lanes) {
    MatchParams mp{};
    mp.B = f.B; mp.h = f.h; mp.w = f.w; mp.dmin = f.dmin; mp.Dd = f.Dd;
    mp.on_lanes = on_lanes ? 1 : 0;
    mp.pass1_only = f.capture ? 1 : 0;
    return mp;
}
// Shape of a fast-kernel launch of n pairs; `small` is also the engine's notion of "few pairs in flight".
inline FastPlan range_fast_plan(const EngineFacts &f, bool on_lanes, int n) { return match_fast_plan(plan_params(f, on_lanes), n, f.cus, f.opt.fast_stack); }

// ---- the launch specs ------------------------------------------------------------------------------------------------------
// The dense exact-order launch of n pairs.  Default radii without the volume: the register-tiled kernel, for few pairs
// (allow_split) in slices of the disparity range that run as separate workgroups and are merged by a launch of their own.
inline ExactLaunch exact_launch(const EngineFacts &f, bool on_lanes, int n, bool allow_split) {
    ExactLaunch x;
    if (!f.default_radii || f.has_volume) {
        x.kernel = f.has_volume ? EXACT_GENERIC_VOLUME : EXACT_GENERIC;
        x.nd_chunk = f.exact_nd;
        x.lds_bytes = f.exact_lds;
        return x;
    }
    x.kernel = EXACT_TILED;
    x.nd_chunk = f.exact2_nd;
    x.lds_bytes = f.exact2_lds;
    x.split = allow_split ? exact_split(f.e2_tiles, n, f.Dd, f.cus) : 1;
    if (x.split > 1) {
        x.slice_floats = (size_t)x.split * SMX_SLICE_WORDS * n * f.h * f.w;
        const int per = (f.Dd + x.split - 1) / x.split;
        if (x.nd_chunk > per) x.nd_chunk = per;          // right tile: never wider than one slice needs
        // 8-wave workgroups (2 rows per thread) unless the launch fills the chip about once AND shares it with the other
        // stream lane's launches (k_match_exact2.h: E2K)
        const long wgs = (long)f.e2_tiles * n * x.split, slots = 2L * f.cus;
        x.rows_per_thread = on_lanes && 2 * wgs > slots && wgs < 2 * slots ? 4 : 2;
    }
    return x;
}

// ... and the lookups of step 6 behind it on the capture route: few pairs share a tile's needed indices between workgroups
// (capture_split), which mostly stage their tiles -- 8 waves do that twice as fast (74 -> 58 us at 1080p)
inline ExactCaptureLaunch exact_capture_launch(const EngineFacts &f, int n, bool allow_split) {
    ExactCaptureLaunch x;
    x.split = allow_split ? capture_split(f.e2_tiles, n, f.Dd, f.cus) : 1;
    x.rows_per_thread = allow_split ? 2 : 4;
    x.nd_chunk = f.exact2_nd;
    x.lds_bytes = exact2_capture_lds_bytes(f.exact2_nd);
    return x;
}

// The fast-kernel launch of a range whose sparse-form shape is pl, in the form the plan asks for (dense: the throughput
// shape, dense_small: the latency shape at 12-row bands).  The dense forms are instantiated for up to 256 disparities at up
// to FA_DENSE_MAX_TH rows (a call that asks for one does not take 32-row bands) and, in the latency shape, for the ranges
// one right-tile chunk holds (257 at pitch 320); a call planned dense beyond that launches the SPARSE instantiation --
// with MatchParams::dense / dense_small still set and without report words (NOTES.md: "Launch specs").
inline FastLaunch fast_launch(const EngineFacts &f, const FastPlan &pl, bool dense, bool dense_small) {
    FastLaunch x;
    x.small = pl.small;
    x.th = pl.th;
    x.pk = fast_pk(f.K * f.K);
    bool dense_here;
    if (pl.small) {
        x.pitch = pl.wide ? 320 : 256;
        dense_here = dense_small && pl.th == FA_TH_SMALL_TALL && f.Dd <= x.pitch - 64 + 1;
    } else {
        x.pitch = fast_tall_pitch(f.Dd);
        x.argb = x.pitch != 320 || f.Dd <= 256;
        if (pl.th == 32 && dense && !f.capture && f.Dd <= 256) x.th = FA_DENSE_MAX_TH;
        dense_here = dense && x.argb && x.th <= FA_DENSE_MAX_TH;
    }
    x.form = f.capture ? FAST_PASS1_ONLY : (!dense_here ? FAST_SPARSE : (pl.small ? FAST_DENSE_SMALL : FAST_DENSE));
    x.stack = pl.stack;              // (match_fast_plan stacks the sparse form only)
    return x;
}

inline FastCaptureLaunch fast_capture_launch(const EngineFacts &f, const FastPlan &pl) {
    return FastCaptureLaunch{pl.small, f.Dd > FA_WIDE_FROM, fast_pk(f.K * f.K)};
}

// The one-launch AUTO kernel at band height th: the grid and tile of the latency-shape fast kernel; its off-grid branch
// splits the range into nsplit slices, with a right-tile chunk no wider than a slice, and needs the larger of the two tiles.
inline AutoLaunch auto_launch(const EngineFacts &f, const MatchParams &mp, int th) {
    AutoLaunch x;
    x.th = th;
    x.wide = fast_small_wide(f.Dd);
    x.pk = fast_pk(f.K * f.K);
    x.nsplit = match_auto_nsplit(mp, th);
    x.nd_chunk = f.exact2_nd;
    const int per = (f.Dd + x.nsplit - 1) / x.nsplit;
    if (x.nd_chunk > per) x.nd_chunk = per;
    x.lds_bytes = x.wide ? fast_lds_bytes<320>(th, f.Dd, true) : fast_lds_bytes<256>(th, f.Dd, true);
    const size_t exact_lds = exact2_lds_floats(x.nd_chunk) * sizeof(float);
    if (exact_lds > x.lds_bytes) x.lds_bytes = exact_lds;
    return x;
}

inline FilterLaunch filter_launch(const EngineFacts &f, const MatchParams &mp, int n) {
    const FilterPlan pl = filter_plan(mp, n, f.cus);
    return FilterLaunch{pl.th, pl.wide, fast_pk(f.filter_unit)};
}

// Steps 1-2.  The two-pixel kernel exists for the gray entries; the block kernel reads a u8 entry's rows with 4-byte loads.
inline PrologueLaunch prologue_launch(const EngineFacts &f, const CallFacts &call) {
    const bool u8 = call.in_mode == IN_GRAY_U8 || call.in_mode == IN_RGB_U8;
    PrologueLaunch x;
    x.in_mode = call.in_mode;
    if (f.prologue_k2 && !is_rgb(call.in_mode)) x.kernel = PROLOGUE_K2;
    else if (f.prologue_k4 && (!u8 || call.u8_aligned)) x.kernel = PROLOGUE_K4;
    return x;
}

// Steps 7-9; on the stream lanes a batch's fill takes 4 pixels per thread (tu_stages.hip: launch_fill).
inline FillLaunch fill_launch(const EngineFacts &f, bool on_lanes, int n) {
    FillLaunch x;
    x.K = f.K;
    x.kernel = f.K == 1 || f.K == 2 || f.K == 4 ? FILL_4 : ((f.K & (f.K - 1)) == 0 ? FILL_POW2 : FILL_GENERIC);
    x.px = on_lanes && n > 4 ? 4 : 8;
    while ((1 << x.log2k) < f.K) x.log2k++;
    return x;
}

inline RangePlan plan_range(const EngineFacts &f, const CallFacts &call, int n, bool whole_call) {
    RangePlan p;
    p.owns_gray = call.in_mode != IN_GRAY_F32;
    p.prologue = prologue_launch(f, call);
    if (f.match_mode == SMX_MATCH_FAST_GRID && !f.fast_ok) {
        p.status = SMX_ERR_UNSUPPORTED;
        p.refusal = "SMX_MATCH_FAST_GRID needs downscale_factor in {1,2,4,8}, ncc radius 1 and "
                    "block-matching radii 1/4/10";
        return p;
    }
    // min_disparity > 0 outside the capture route (dmin > Dd, or other radii): only the generic exact-order
    // kernel still materialises the aggregated volume step 6 then gathers from (rule S6)
    if (f.has_volume && f.match_mode == SMX_MATCH_FAST_GRID) {
        p.status = SMX_ERR_UNSUPPORTED;
        p.refusal = "SMX_MATCH_FAST_GRID cannot serve min_disparity/K > disparity count or "
                    "non-default radii with min_disparity > 0 (aggregated volume needed)";
        return p;
    }
    const bool rgb = is_rgb(call.in_mode);
    // The aggregation kernel(s) a call of this entry enqueues: SMX_MATCH_EXACT_ORDER, SMX_MATCH_FAST_GRID, or SMX_MATCH_AUTO
    // when both are enqueued and the device-side grid flag selects.
    p.mode = f.match_mode;
    if (f.has_volume) p.mode = SMX_MATCH_EXACT_ORDER;
    if (p.mode == SMX_MATCH_AUTO) {
        if (!f.fast_ok) p.mode = SMX_MATCH_EXACT_ORDER;
        else if (call.in_mode == IN_GRAY_U8) p.mode = SMX_MATCH_FAST_GRID;   // u8 is on the grid
        // gray computed from RGB (0.2989 R + 0.5870 G + 0.1140 B in float32) is practically never on the
        // grid, not even for R = G = B: do not enqueue the fast kernel as a gated alternative at all (the
        // exact-order kernel is correct for any input, so this is a launch saved, never a different result)
        else if (rgb) p.mode = SMX_MATCH_EXACT_ORDER;
    }
    const MatchParams mp = plan_params(f, call.on_lanes);
    p.fast = match_fast_plan(mp, n, f.cus, f.opt.fast_stack);
    const bool small = p.fast.small;
    // dmin > 0 (capture route): the match kernels stop after the arg-max; a sparse second kernel looks up the
    // three aggregated costs step 6 reads (k_match_capture.h; the workgroup that owns pixel 0 of a pair evaluates that pixel's
    // out-of-range lookups directly, k_capture_pixel0.h)
    p.capture_follows = f.capture;

    if (p.mode == SMX_MATCH_EXACT_ORDER && f.filter_ok && rgb && !small && f.default_radii && call.route.use_filter) {
        // the filtered route (k_match_filter.h): a cheap pass over all disparities on the inputs rounded to the grid marks,
        // per exact-order tile, the disparities that can still hold the maximum; only those are evaluated in the
        // reference's order.  Pairs whose gray leaves [0, 255] (f32 RGB only; flag from the prologue) take the dense kernel.
        p.route = AGG_FILTERED;
        p.gated_dense_first = call.in_mode == IN_RGB_F32;      // (gate 2 on the range flag, below)
        p.filter = filter_launch(f, mp, n);
    } else if (p.mode == SMX_MATCH_EXACT_ORDER) {
        p.route = AGG_EXACT;
        // (the disparity split is for calls of a few pairs; its slice buffer is not divided between halves)
        p.exact_split = whole_call;
    } else if (p.mode == SMX_MATCH_FAST_GRID) {
        p.route = AGG_FAST;
    } else {
        // AUTO, few pairs in flight, the last reported call on the grid: one launch that branches on the device-side
        // flag (k_match_auto.h).  Its exact-order branch (the disparity-split register-tiled kernel on the fast kernel's
        // grid, merged by the last workgroup of a tile) is ~1.4 x slower than the two gated launches, so those serve
        // once a call has reported off-grid input -- and as long as nothing has been reported at all: an engine's first calls.
        const bool one_launch = f.default_radii && small && call.route.grid_hint == 0 && !f.capture && !f.has_volume && f.has_tickets() &&
                                f.has_slices() && match_auto_small_applicable(mp, p.fast.th, n, f.slices_floats);
        if (one_launch) {
            p.route = AGG_AUTO_ONE_LAUNCH;
            p.auto_launch = auto_launch(f, mp, p.fast.th);
        } else {
            p.route = AGG_AUTO_GATED;
            // the disparity split (and its merge launch) only for few pairs that are known to be off the grid; for the
            // gated alternative of on-grid batches it would be pure overhead
            p.exact_split = whole_call && small && call.route.grid_hint != 0;
        }
    }

    // form of the fast kernel
    if (p.has_fast_launch() && !mp.pass1_only && f.Dd <= FA_BITWORDS * 32) {
        const bool tall12 = small && p.fast.th == FA_TH_SMALL_TALL;
        if (!small || tall12) {                  // (8- / 10-row bands: no dense form)
            // its sparse form reports, unless a form is forced: a sample of the launch, at most four pairs, and only if their
            // waves fit the counter's 24-bit window field
            if (!(tall12 && f.opt.fast_dense_small == 1) && f.fast_words && f.opt.fast_dense < 0) {
                p.stride = n > 4 ? (n + 3) / 4 : 1;
                const long wgs_pair = tall12 ? (long)((f.w + FA_VALID - 1) / FA_VALID) * ((f.h + p.fast.th - 1) / p.fast.th)      // (an upper bound of the reports per pair)
                                             : (long)((f.w + FA_VALID * FA_WAVES - 1) / (FA_VALID * FA_WAVES)) * ((f.h + 23) / 24) * FA_WAVES;
                p.reports = ((n + p.stride - 1) / p.stride) * wgs_pair < (1L << 23);
            }
            const bool dense = tall12 && f.opt.fast_dense_small >= 0 ? f.opt.fast_dense_small == 1 : call.route.fast_dense;
            if (dense) (tall12 ? p.dense_small : p.dense) = true;
            else p.fill_publishes = p.reports;
        }
    }
    if (p.dense && p.fast.stack > 1) {           // the stacked bands have no dense form: a dense call takes the plan without them
        MatchParams md = mp;
        md.dense = 1;
        p.fast = match_fast_plan(md, n, f.cus, f.opt.fast_stack);
    }

    if (p.route == AGG_FILTERED || p.route == AGG_EXACT || p.route == AGG_AUTO_GATED) {
        p.exact = exact_launch(f, call.on_lanes, n, p.exact_split);
        if (p.capture_follows) p.exact_capture = exact_capture_launch(f, n, p.exact_split);
    }
    if (p.route == AGG_FAST || p.route == AGG_AUTO_GATED) {
        p.fast_launch = fast_launch(f, p.fast, p.dense, p.dense_small);
        if (p.capture_follows) p.fast_capture = fast_capture_launch(f, p.fast);
    }
    // the gates: a launch runs for every pair (0), for the pairs whose flag is clear (1) or for those whose flag is set (2)
    if (p.route == AGG_FILTERED) {
        p.exact.gate = 2;
        p.exact.gate_flag = GATE_RANGE_FLAG;
    } else if (p.route == AGG_AUTO_GATED) {   // the grid flag lets exactly one of the two [pairs of] launches do the work
        p.exact.gate = p.exact_capture.gate = 2;
        p.fast_launch.gate = p.fast_capture.gate = 1;
    }

    // step 6: integer-valued gray -> v_sad_u8 kernel; otherwise the float kernel (same results)
    p.refine.kt = f.kt;
    p.refine.sad_exact = f.sad_exact;
    if (f.kt == 0 || !f.has_u8_planes() || rgb) {
        p.refine.kind = REFINE_FLOAT;
        p.refine.apron = p.owns_gray && f.gpadl > 0 && call.in_mode != IN_GRAY_U8;   // the u8 gray prologue writes no float aprons
    } else if (call.in_mode == IN_GRAY_U8) {
        // u8 is integer-valued by construction; the prologue wrote the padded copy.  Batches: four pooled rows per
        // thread share their row SADs (k_refine_int_v)
        p.refine.kind = n > 4 ? REFINE_INT_V : REFINE_INT;
    } else if (n <= 4) {   // f32 gray, few pairs: one launch picks per pair (k_refine_auto) and reports the grid flag
        p.refine.kind = REFINE_AUTO;
        p.refine_reports_grid = whole_call;
    } else {   // f32 gray batches: the prologue wrote u8 copies and the per-pair integrality flag; one launch
        // branches on it per pair (k_refine_auto_v: a gated-out launch of the float kernel still has to be placed on
        // a chip the other lane fills, and the lane's chain waits for it)
        p.refine.kind = REFINE_AUTO_V;
    }
    p.fill = fill_launch(f, call.on_lanes, n);
    p.writes_units = p.route != AGG_EXACT && p.route != AGG_FILTERED;     // (those two read the f32 planes only)
    return p;
}

// ---- from spec to the launch's parameters -------------------------------------------------------------------------------------
// What the aggregation launches of a range share, bound once by enqueue_range: buffers, shape, radii, epoch, the lane's slice
// region and the tickets in `mp` (flags: the grid flag, gate 0, unit K^2), and the two words only some launches get.
struct RangeParams {
    MatchParams mp{};
    const int *range_flags = nullptr;            // [B] == epoch: the pair's gray leaves [0, 255] (the prologue's second flag word)
    unsigned long long *fast_stats = nullptr;    // this lane's counter of the sparse fast kernel's report
};
inline MatchParams exact_params(const RangeParams &b, const ExactLaunch &x, int n) {
    MatchParams p = b.mp;
    p.gate = x.gate;
    if (x.gate_flag == GATE_RANGE_FLAG) p.flags = b.range_flags;
    p.nd_chunk = x.nd_chunk;
    if (x.split > 1) {
        p.nsplit = x.split;
        p.pairs = n;
        p.tickets = nullptr;                     // merged by a launch of its own, not by a tile's last slice
    }
    return p;
}
inline MatchParams exact_capture_params(const RangeParams &b, const ExactCaptureLaunch &x) {
    MatchParams p = b.mp;
    p.gate = x.gate;
    p.nd_chunk = x.nd_chunk;
    p.nsplit = x.split;
    return p;
}
// the fast kernel in the plan's form; the sparse form's report is published by the range's fill launch
inline MatchParams fast_params(const RangeParams &b, const RangePlan &pl, int gate) {
    MatchParams p = b.mp;
    p.gate = gate;
    p.dense = pl.dense ? 1 : 0;
    p.dense_small = pl.dense_small ? 1 : 0;
    if (pl.fill_publishes) {
        p.fast_stats = b.fast_stats;
        p.fast_stride = pl.stride;
    }
    return p;
}
// the off-grid branch: slices, a right-tile chunk no wider than a slice, records of n pairs
inline MatchParams auto_params(const RangeParams &b, const RangePlan &pl, int n) {
    MatchParams p = fast_params(b, pl, 0);
    p.nsplit = pl.auto_launch.nsplit;
    p.pairs = n;
    p.nd_chunk = pl.auto_launch.nd_chunk;
    return p;
}
inline MatchParams filter_params(const RangeParams &b, const EngineFacts &f) {
    MatchParams p = b.mp;
    p.unit = (float)f.filter_unit;
    return p;
}
inline MatchParams sparse_params(const RangeParams &b, const EngineFacts &f) {   // (launch_exact2_sparse has no spec: one instantiation)
    MatchParams p = b.mp;
    p.nd_chunk = f.exact2_nd;
    return p;
}

// Which of the two content switches a call can report to on its default route (filter allowed, sparse form), from the
// plans of its range(s) (n1 = 0: an unsplit call).  A switch follows, and is probed by, calls of its own kind only.
inline CallKind call_kind(const EngineFacts &f, int in_mode, bool on_lanes, int n0, int n1) {
    CallKind k{};
    CallFacts call;
    call.in_mode = in_mode;
    call.on_lanes = on_lanes;
    for (int n : {n0, n1}) {
        if (n < 1) continue;
        const RangePlan p = plan_range(f, call, n, n1 < 1);
        if (p.status != SMX_OK) continue;
        if (p.route == AGG_FILTERED && f.filter_words) k.filter_reports = true;
        if (p.has_fast_launch() && p.reports) k.fast_reports = true;
    }
    return k;
}

// What smx_get_match_geometry reports for a fast-kernel launch of n pairs: the plan of the sparse form (FastPlan), not the
// instantiation a dense call launches (RangePlan::fast_launch).
inline void match_geometry(const EngineFacts &f, bool on_lanes, int n, smx_match_geometry *g) {
    if (!f.fast_ok) {
        g->kernel = SMX_KERNEL_EXACT_ONLY;
        return;
    }
    const FastPlan pl = range_fast_plan(f, on_lanes, n);
    g->kernel = pl.small ? SMX_KERNEL_FAST_SPLIT : SMX_KERNEL_FAST_WINDOW;
    g->band_rows = pl.th * pl.stack;
    g->waves_per_workgroup = pl.small ? FA_DS_WAVES : FA_WAVES;
    const int cols_per_wg = FA_VALID * (pl.small ? 1 : FA_WAVES);
    const long wgs = (long)((f.w + cols_per_wg - 1) / cols_per_wg) * ((f.h + g->band_rows - 1) / g->band_rows);
    g->rows_marched = g->band_rows + 22;
    g->workgroups = (int)(wgs * n);
    const long waves = wgs * g->waves_per_workgroup;
    // the disparity-split kernel spends its 4 waves on one window: a quarter of the range each
    const double lane_rows = (double)waves * 64.0 * g->rows_marched / (g->kernel == SMX_KERNEL_FAST_SPLIT ? (double)FA_DS_WAVES : 1.0);
    g->useful_fraction = (double)f.h * f.w / lane_rows;
    g->columns_per_wave = (double)f.w * ((f.h + g->band_rows - 1) / g->band_rows) /
                          ((double)waves / (g->kernel == SMX_KERNEL_FAST_SPLIT ? (double)FA_DS_WAVES : 1.0));
}

}  // namespace smx
