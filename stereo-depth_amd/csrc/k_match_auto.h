// k_match_auto.h -- SMX_MATCH_AUTO for a few f32 gray pairs in ONE launch.
//
// In AUTO mode the prologue decides per pair, on the device, whether the pooled images lie on the
// exact 1/K^2 grid; the engine then enqueues the FAST_GRID kernel and the exact-order kernel and each
// exits for the pairs the flag gives to the other.  For large batches the idle launch is noise, at
// single-pair latency it is ~6 us of ~45.  This kernel is launched on the grid of the
// disparity-split fast kernel and branches on the flag per workgroup: on the grid it runs that
// kernel's body; off the grid its workgroups become the disparity-split REGISTER-TILED exact-order kernel
// (k_match_exact2.h, the 8-wave form: 2 rows per thread, 117 registers -- it fits this kernel's register
// budget and block size): workgroup lin takes slice lin % nsplit of 16x128 tile lin / nsplit, writes
// its partial arg-max records, and the last workgroup of a tile to arrive (a device-scope ticket per tile, reset by
// the workgroup that merges) merges the tile's slices -- no merge launch.
// Rounds 2 - 3 ran the generic exact-order body here (68 registers: all that fitted beside the 4-row register-tiled
// one's 191), 3 x slower per pixel and unsplit: the first off-grid call after on-grid ones took 700 us at C2; this
// form takes ~150.  k_refine_auto reports the grid flag to the host (RefineParams::grid_hint), and while the last
// report says "off the grid" the engine enqueues the two gated launches instead, which are faster still.
#pragma once
#include "k_match_exact2.h"
#include "k_match_fast.h"

namespace smx {

template <int TH, int PR, int PK16>
__global__ __launch_bounds__(64 * FA_DS_WAVES, TH >= FA_TH_SMALL_TALL ? 2 : FA_DS_OCC) void k_match_auto_small(MatchParams p) {
    const BlockIdx3 blk = xcd_block_index();
    const int b = blk.z;
    if (p.flags[b] != p.epoch) {                               // uniform per workgroup
        if constexpr (TH == FA_TH_SMALL_TALL) {
            if (p.dense_small && p.Dd <= PR - 64 + 1) {        // launch-uniform: the dense form of the latency shape (k_match_fast.h)
                match_fast_body<TH, PR, false, true, PK16, false, true>(p, blk);
                return;
            }
        }
        match_fast_body<TH, PR, false, true, PK16>(p, blk);
        return;
    }
    // off the grid: p.nsplit slices per 16x128 tile (a power of two, nsplit * tiles <= workgroups per pair: match_auto_nsplit)
    static_assert(64 * FA_DS_WAVES == E2K<2>::THREADS, "the off-grid branch is the 8-wave exact-order body");
    const int tiles_x = (p.w + E2_TW - 1) / E2_TW, tiles = tiles_x * ((p.h + E2_TH - 1) / E2_TH);
    const int lin = (int)(blk.x + gridDim.x * blk.y);
    if (lin >= tiles * p.nsplit) return;                     // uniform per workgroup
    const int tile = lin / p.nsplit, sp = lin - tile * p.nsplit;
    match_exact2_body<true, 2>(p, tile % tiles_x, tile / tiles_x, b, sp);
    e2_merge_by_last_arriver<64 * FA_DS_WAVES>(p, b, tile, tiles, tiles_x);
}

// slices per tile of the off-grid branch: as many as the workgroups of the fast grid can serve (a power of two up to 8, at
// least 4 disparities per slice)
inline int match_auto_nsplit(const MatchParams &p, int th) {
    const long fast_wgs = (long)((p.w + FA_VALID - 1) / FA_VALID) * ((p.h + th - 1) / th);
    const long tiles = (long)((p.w + E2_TW - 1) / E2_TW) * ((p.h + E2_TH - 1) / E2_TH);
    int ns = 1;
    while (ns < 8 && 2L * ns * tiles <= fast_wgs && p.Dd / (2 * ns) >= 4) ns *= 2;
    return ns;
}

// Floats of slice records the off-grid branch of a one-launch call of n pairs writes: [nsplit][SMX_SLICE_WORDS][n][h][w].
// One rule for the buffer and the launch: slice_region_floats sizes each stream lane's region with it, and
// match_auto_small_applicable refuses a call whose records do not fit (it takes the two gated launches instead).
inline size_t match_auto_slice_floats(const MatchParams &p, int n, int th) {
    return (size_t)match_auto_nsplit(p, th) * (size_t)n * SMX_SLICE_WORDS * (size_t)p.h * (size_t)p.w;
}

// Floats of one stream lane's region of the slice buffer (smx_create; two small calls may be in flight at once): the
// largest disparity split exact_launch (smx_plan.h) can plan (calls of up to 4 pairs) and, if the engine can take the one-launch AUTO
// kernel (one_launch), the records of its calls of up to 16 pairs in the latency shape, on a caller's stream or on the
// lanes.  Larger calls that would need more room take the two gated launches, whose split is 1 beyond 4 pairs.
// p: the engine's h, w and Dd; cus: the device's CU count.
inline size_t slice_region_floats(MatchParams p, int B, int cus, bool one_launch) {
    const int tiles = ((p.w + E2_TW - 1) / E2_TW) * ((p.h + E2_TH - 1) / E2_TH);
    const size_t hw = (size_t)p.h * p.w;
    size_t floats = 0;
    for (int n = 1; n <= B && n <= 4; ++n) {
        const int sp = exact_split(tiles, n, p.Dd, cus);
        const size_t need = (size_t)sp * n * SMX_SLICE_WORDS * hw;
        if (sp > 1 && need > floats) floats = need;
    }
    if (one_launch) {
        p.pass1_only = 0;                       // (the one-launch kernel never serves the capture route)
        for (int n = 1; n <= B && n <= 16; ++n) {
            for (int lanes = 0; lanes < 2; ++lanes) {
                p.on_lanes = lanes;
                const FastPlan pl = match_fast_plan(p, n, cus);
                const size_t need = pl.small ? match_auto_slice_floats(p, n, pl.th) : 0;
                if (need > floats) floats = need;
            }
        }
    }
    return floats;
}

// Dynamic-LDS limit the engine raises these kernels to once per device (max of the fast split tile and the 64 KB exact tile;
// the split tile's needed-set table grows with the range: 73 KB + 32 B per disparity up to 2048 disparities at 8-row bands,
// 97 KB + 32 B at 12-row bands -- those run one workgroup per CU by design).
constexpr int MATCH_AUTO_LDS_CAP = 128 * 1024;

// workgroups per pair of the disparity-split fast kernel / of the exact-order kernel; ranges whose tile would not fit
// the raised limit (more than ~780 disparities) take the two gated launches instead
// th: the band height match_fast_plan chose for this call of n pairs; slices_floats: the floats of this lane's region of
// the slice buffer (the records of the off-grid branch must fit it)
// (whether the engine has the buffers at all -- no capture route, no volume, tickets and slices allocated -- is the
// planner's part of the gate: smx_plan.h)
inline bool match_auto_small_applicable(const MatchParams &p, int th, int n, size_t slices_floats) {
    const long fast_wgs = (long)((p.w + FA_VALID - 1) / FA_VALID) * ((p.h + th - 1) / th);
    const long tiles = (long)((p.w + E2_TW - 1) / E2_TW) * ((p.h + E2_TH - 1) / E2_TH);
    const size_t lds = fast_small_wide(p.Dd) ? fast_lds_bytes<320>(th, p.Dd, true) : fast_lds_bytes<256>(th, p.Dd, true);
    return fast_wgs >= tiles && lds <= (size_t)MATCH_AUTO_LDS_CAP && match_auto_slice_floats(p, n, th) <= slices_floats;
}

// From launch spec (smx_plan.h: auto_launch) to instantiation; p.nsplit, p.pairs and p.nd_chunk are the spec's.
template <int TH, int PR>
inline void launch_match_auto_small_t(const AutoLaunch &al, const MatchParams &p, int n, hipStream_t s) {
    const dim3 grid((p.w + FA_VALID - 1) / FA_VALID, (p.h + TH - 1) / TH, n), block(64 * FA_DS_WAVES);
    if (al.pk == 2) hipLaunchKernelGGL((k_match_auto_small<TH, PR, 2>), grid, block, al.lds_bytes, s, p);
    else if (al.pk == 1) hipLaunchKernelGGL((k_match_auto_small<TH, PR, 1>), grid, block, al.lds_bytes, s, p);
    else hipLaunchKernelGGL((k_match_auto_small<TH, PR, 0>), grid, block, al.lds_bytes, s, p);
}

inline void launch_match_auto_small(const AutoLaunch &al, const MatchParams &p, int n, hipStream_t s) {
    if (al.th == FA_TH_SMALL_TALL) {
        if (!al.wide) launch_match_auto_small_t<FA_TH_SMALL_TALL, 256>(al, p, n, s);
        else launch_match_auto_small_t<FA_TH_SMALL_TALL, 320>(al, p, n, s);
    } else if (al.th == FA_TH_SMALL_MID) {
        if (!al.wide) launch_match_auto_small_t<FA_TH_SMALL_MID, 256>(al, p, n, s);
        else launch_match_auto_small_t<FA_TH_SMALL_MID, 320>(al, p, n, s);
    } else {
        if (!al.wide) launch_match_auto_small_t<FA_TH_SMALL, 256>(al, p, n, s);
        else launch_match_auto_small_t<FA_TH_SMALL, 320>(al, p, n, s);
    }
}

template <int TH>
inline hipError_t match_auto_raise_lds_caps_t(int cap_bytes) {
    const void *fns[] = {reinterpret_cast<const void *>(&k_match_auto_small<TH, 256, 2>), reinterpret_cast<const void *>(&k_match_auto_small<TH, 256, 1>),
                         reinterpret_cast<const void *>(&k_match_auto_small<TH, 256, 0>), reinterpret_cast<const void *>(&k_match_auto_small<TH, 320, 2>),
                         reinterpret_cast<const void *>(&k_match_auto_small<TH, 320, 1>), reinterpret_cast<const void *>(&k_match_auto_small<TH, 320, 0>),
                         // the plain latency-shape kernels of the same band height (FAST_GRID mode, u8 entry, gated AUTO launches)
                         reinterpret_cast<const void *>(&k_match_fast<TH, 256, false, true, 2, false>), reinterpret_cast<const void *>(&k_match_fast<TH, 256, false, true, 1, false>),
                         reinterpret_cast<const void *>(&k_match_fast<TH, 256, false, true, 0, false>), reinterpret_cast<const void *>(&k_match_fast<TH, 320, false, true, 2, false>),
                         reinterpret_cast<const void *>(&k_match_fast<TH, 320, false, true, 1, false>), reinterpret_cast<const void *>(&k_match_fast<TH, 320, false, true, 0, false>),
                         reinterpret_cast<const void *>(&k_match_fast<TH, 256, true, true, 2, false>), reinterpret_cast<const void *>(&k_match_fast<TH, 256, true, true, 1, false>),
                         reinterpret_cast<const void *>(&k_match_fast<TH, 256, true, true, 0, false>), reinterpret_cast<const void *>(&k_match_fast<TH, 320, true, true, 2, false>),
                         reinterpret_cast<const void *>(&k_match_fast<TH, 320, true, true, 1, false>), reinterpret_cast<const void *>(&k_match_fast<TH, 320, true, true, 0, false>)};
    for (const void *f : fns) {
        hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, cap_bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
inline hipError_t match_auto_raise_lds_caps(int cap_bytes) {
    if (hipError_t e = match_auto_raise_lds_caps_t<FA_TH_SMALL>(cap_bytes); e != hipSuccess) return e;
    if (hipError_t e = match_auto_raise_lds_caps_t<FA_TH_SMALL_MID>(cap_bytes); e != hipSuccess) return e;
    return match_auto_raise_lds_caps_t<FA_TH_SMALL_TALL>(cap_bytes);
}

}  // namespace smx
