// k_tsdf_merge.h -- one TSDF volume's state written into another, in place (smx_tsdf_merge): a region of a source volume is
// paired with the destination voxels it lies on, and every destination voxel whose source has been measured (W1 > 0) takes
// the source's words (where the destination has none) or, in AVERAGE mode, the weighted mean of both, exactly in
// smx_tsdf_integrate's form.  The rule is in include/stereo_mi355x.h; tests/tsdf_merge_ref.py restates it in NumPy.
// What restores a spilled box when the camera returns (FILL) and what joins two volumes fused from different frames
// (AVERAGE).
//
// The shape is k_tsdf_window.h's: one short-lived wave per destination row (k, j) OF THE OVERLAP (the host clips the region
// to the destination grid, so every voxel of a row has a source and a destination), four rows per workgroup, the two row
// bases decided once from wave-uniform values.  Inside a row a lane owns quads of 4 voxels, two per trip; the quads start at
// the first 16-byte boundary of the destination's WEIGHT row (the three destination arrays share that phase whenever
// their bases are 16-byte aligned, which every allocator gives), so the destination's accesses are aligned dwordx4 and
// the source's dwordx4 at the 4-byte alignment the placement leaves.  The up to 3 + 3 voxels before the first and after
// the last quad are single words.
// What the window does not have: the source WEIGHT quad is loaded first, and a quad with no W1 > 0 -- most of a fused
// volume is unmeasured space -- loads and stores nothing else.  Then the destination's weights; in FILL mode a quad whose
// destination voxels are all measured stops there too, and one whose voxels are all replaced never reads the
// destination's tsdf and colour.  A quad in which no word changes is not stored.  Every voxel has one owner lane, so the
// update in place is safe.  No atomics, no workspace, no LDS.
#pragma once
#include <cstddef>

#include "k_camera.h"

namespace smx {

constexpr int MRG_WAVES = 4;           // waves = rows per workgroup
constexpr int MRG_FILL = 0, MRG_AVERAGE = 1;   // SMX_TSDF_MERGE_*

struct TsdfMergeArgs {
    int nx, ny;                        // destination row and slab pitch (voxels, rows)
    int sx, sy;                        // the source's
    int dx, dy, dz;                    // first destination voxel of the overlap
    int ox, oy, oz;                    // the overlap's dims, all >= 1
    int x0, y0, z0;                    // source voxel (0, 0, 0) in destination voxels
    int mode;
    float max_weight;
    unsigned *dst[3];                  // tsdf, weight, color words; dst[2] / src[2] NULL: no colour
    const unsigned *src[3];
};

typedef unsigned mrg_quad __attribute__((ext_vector_type(4)));
typedef unsigned mrg_quad_a4 __attribute__((ext_vector_type(4), aligned(4)));

// The rule for one pair in AVERAGE mode with W0 > 0 and W1 > 0: every step one float32 operation, integrate's form.
__device__ __forceinline__ void merge_average(unsigned &t0, unsigned &w0, unsigned &c0, unsigned t1, unsigned w1,
                                              unsigned c1, float max_weight, bool colour) {
    const float T0 = __uint_as_float(t0), W0 = __uint_as_float(w0), T1 = __uint_as_float(t1), W1 = __uint_as_float(w1);
    const float den = W0 + W1;
    t0 = __float_as_uint(((T0 * W0) + (T1 * W1)) / den);
    w0 = __float_as_uint(fminf(den, max_weight));
    if (colour) {
        unsigned out = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const float C0 = (float)((c0 >> (8 * ch)) & 255u), C1 = (float)((c1 >> (8 * ch)) & 255u);
            out |= colour_byte(((C0 * W0) + (C1 * W1)) / den) << (8 * ch);
        }
        c0 = out;
    }
}

__device__ __forceinline__ bool merge_measured(unsigned w) { return __uint_as_float(w) > 0.0f; }   // NaN fails

// a single voxel: the head and the tail of a row
__device__ __forceinline__ void merge_word(const TsdfMergeArgs &a, unsigned *const d[3], const unsigned *const s[3], int i) {
    const unsigned w1 = s[1][i];
    if (!merge_measured(w1)) return;
    unsigned w0 = d[1][i];
    const bool colour = d[2] != nullptr;
    if (!merge_measured(w0)) {
        d[0][i] = s[0][i];
        d[1][i] = w1;
        if (colour) d[2][i] = s[2][i];
        return;
    }
    if (a.mode == MRG_FILL) return;
    unsigned t0 = d[0][i], c0 = colour ? d[2][i] : 0u;
    merge_average(t0, w0, c0, s[0][i], w1, colour ? s[2][i] : 0u, a.max_weight, colour);
    d[0][i] = t0;
    d[1][i] = w0;
    if (colour) d[2][i] = c0;
}

__device__ __forceinline__ mrg_quad merge_load_src(const unsigned *p) {
    return __builtin_nontemporal_load(reinterpret_cast<const mrg_quad_a4 *>(p));
}

// One quad of a row whose source weights w1 are loaded: voxels i .. i + 3 of d[t] and s[t].
__device__ __forceinline__ void merge_quad(const TsdfMergeArgs &a, unsigned *const d[3], const unsigned *const s[3], int i,
                                           const mrg_quad w1) {
    const bool colour = d[2] != nullptr;
    const bool m1[4] = {merge_measured(w1.x), merge_measured(w1.y), merge_measured(w1.z), merge_measured(w1.w)};
    if (!(m1[0] || m1[1] || m1[2] || m1[3])) return;                // unmeasured source: nothing else is touched
    const mrg_quad w0 = *reinterpret_cast<const mrg_quad *>(d[1] + i);
    const bool m0[4] = {merge_measured(w0.x), merge_measured(w0.y), merge_measured(w0.z), merge_measured(w0.w)};
    bool take[4], keep = true, all = true;                            // take: the destination becomes the source
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        take[c] = m1[c] && !m0[c];
        keep = keep && !take[c];
        all = all && take[c];
    }
    if (a.mode == MRG_FILL && keep) return;                         // every measured pair keeps the destination
    const mrg_quad t1 = merge_load_src(s[0] + i);
    mrg_quad c1 = {0u, 0u, 0u, 0u};
    if (colour) c1 = merge_load_src(s[2] + i);
    mrg_quad t0 = t1, c0 = c1;                                        // all four replaced: the destination is not read
    if (!all) {
        t0 = *reinterpret_cast<const mrg_quad_a4 *>(d[0] + i);
        if (colour) c0 = *reinterpret_cast<const mrg_quad_a4 *>(d[2] + i);
    }
    mrg_quad t = t0, w = w0, c = c0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        if (take[e]) {
            t[e] = t1[e], w[e] = w1[e], c[e] = c1[e];
        } else if (a.mode == MRG_AVERAGE && m1[e]) {                 // m0[e] holds: else take[e]
            unsigned te = t0[e], we = w0[e], ce = c0[e];
            merge_average(te, we, ce, t1[e], w1[e], c1[e], a.max_weight, colour);
            t[e] = te, w[e] = we, c[e] = ce;
        }
    }
    // a quad in which no word changes (AVERAGE of equal values below the cap) is not stored
    if (!all) {
        bool same = w.x == w0.x && w.y == w0.y && w.z == w0.z && w.w == w0.w;
        same = same && t.x == t0.x && t.y == t0.y && t.z == t0.z && t.w == t0.w;
        same = same && c.x == c0.x && c.y == c0.y && c.z == c0.z && c.w == c0.w;
        if (same) return;
    }
    __builtin_nontemporal_store(t, reinterpret_cast<mrg_quad_a4 *>(d[0] + i));
    __builtin_nontemporal_store(w, reinterpret_cast<mrg_quad *>(d[1] + i));
    if (colour) __builtin_nontemporal_store(c, reinterpret_cast<mrg_quad_a4 *>(d[2] + i));
}

// One row of `count` pairs by one wave: d[t] + i is paired with s[t] + i.  A lane takes two quads per trip, 64 quads
// apart, and loads both source weight quads before it looks at either: a row of up to 512 voxels is one trip.
__device__ __forceinline__ void merge_row(const TsdfMergeArgs &a, unsigned *const d[3], const unsigned *const s[3],
                                          int count, int lane) {
    const int to_boundary = (int)((0u - (unsigned)((uintptr_t)d[1] >> 2)) & 3u);
    const int head = to_boundary < count ? to_boundary : count;
    const int quads = (count - head) >> 2;
    for (int q = lane; q < quads; q += 128) {
        const int i = head + 4 * q;
        const bool second = q + 64 < quads;
        const mrg_quad wa = merge_load_src(s[1] + i);
        mrg_quad wb = {0u, 0u, 0u, 0u};
        if (second) wb = merge_load_src(s[1] + i + 256);
        merge_quad(a, d, s, i, wa);
        if (second) merge_quad(a, d, s, i + 256, wb);
    }
    const int tail = head + 4 * quads;                               // [0, head) and [tail, count): single voxels
    if (lane < head + (count - tail)) merge_word(a, d, s, lane < head ? lane : tail + (lane - head));
}

__global__ __launch_bounds__(64 * MRG_WAVES) void k_tsdf_merge(const TsdfMergeArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rows = (unsigned)a.oy * (unsigned)a.oz;           // <= 2^24
    const unsigned r = blockIdx.x * MRG_WAVES + wave;                // this wave's row of the overlap
    if (r >= rows) return;
    const unsigned k = r / (unsigned)a.oy, j = r - k * (unsigned)a.oy;
    const int y = a.dy + (int)j, z = a.dz + (int)k;                  // the destination row
    const size_t drow = voxel_index(z, y, a.dx, a.ny, a.nx);
    // voxel_index of the source row, written out: as a call its three differences move in the device code
    const size_t srow = ((size_t)(z - a.z0) * a.sy + (y - a.y0)) * (size_t)a.sx + (a.dx - a.x0);
    unsigned *d[3] = {a.dst[0] + drow, a.dst[1] + drow, a.dst[2] ? a.dst[2] + drow : nullptr};
    const unsigned *s[3] = {a.src[0] + srow, a.src[1] + srow, a.src[2] ? a.src[2] + srow : nullptr};
    merge_row(a, d, s, a.ox, lane);
}

}  // namespace smx
