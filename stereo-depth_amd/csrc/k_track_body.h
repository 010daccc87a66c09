// k_track_body.h -- the launches of camera tracking, written once over the rule that is tracked: the three kernel bodies
// and the launcher that fills the common record and runs the schedule.  k_track.h instantiates them for the geometric
// rule (smx_track_camera), k_track_photo.h for the joint one (smx_track_camera_photometric) and k_track_pyramid.h for
// the joint one read from pyramids (smx_track_camera_pyramid).
//
// A rule R holds
//   Args                 its kernel argument record, and common(a): the TrackArgs in it
//   SLOTS, BUTTERFLY     the sums a pixel adds to, and how many of them the accumulate's butterfly reduces (the rest are
//                        unused slots that stay +0.0)
//   CHUNKS, STACK        the combine's chunks of consecutive partials per triple, 1024 / CHUNKS lanes each of which the
//                        first SLOTS work, and its levels above a leaf of eight
//   pixel, begin, finish the rule itself (k_track_rule.h, k_track_photo_rule.h)
//
// An iteration is two launches.  Accumulate: one wave per tile of 64 x TRK_ROWS selected pixels, one lane per column
// walking its rows top to bottom with the float64 sums (and the count of accepted pixels) in registers; the 64 columns
// are reduced by an xor butterfly -- lanes l and l^1 first, every lane ending with the same bits as an adjacent-pairs
// tree since a + b = b + a -- and the four tiles of a workgroup through LDS, (t0 + t1) + (t2 + t3), which is two levels
// of the tile tree.  Combine: one workgroup per triple finishes the tile tree over the groups of four (thread = (chunk of
// consecutive partials, slot): a chunk's tree with a stack of one value per level in LDS, then the chunks' tree), and its
// first thread ends the iteration: the solve, the pose, the outputs and the stop flags.  A chunk is a power of two of
// consecutive partials, so chunk trees followed by the chunks' tree are the header's adjacent-pairs tree whatever the
// number of chunks.  Both return at once for a triple that has stopped.  No atomics, and nothing passes between
// workgroups inside a launch: what one launch writes the next one reads.
#pragma once
#include <cstring>

#include "k_track_rule.h"
#include "smx_launch.h"

namespace smx {

// The bodies take the record by value, as a kernel does, and are static, so that their LDS arrays are the kernel's own:
// the compiler then reads the record's fields and lays the arrays out as it does for a kernel written out in full.

// one thread per triple: state and the outputs of "no iteration ran"
template <class R> static __device__ __forceinline__ void track_begin_body(const typename R::Args ra) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < R::common(ra).n) R::begin(ra, f);
}

// grid (groups, min(n, 65535)); wave w of workgroup b owns tile 4 b + w of the selected grid, in row-major order
template <class R> static __device__ __forceinline__ void track_accum_body(const typename R::Args ra) {
    constexpr int SLOTS = R::SLOTS;
    const TrackArgs &a = R::common(ra);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double red[TRK_WAVES][SLOTS];
    for (int f = blockIdx.y; f < a.n; f += gridDim.y) {
        const TrackState &st = a.state[f];
        if (st.done) continue;                                        // the same for the whole workgroup
        double acc[SLOTS];
#pragma unroll
        for (int k = 0; k < SLOTS; ++k) acc[k] = 0.0;
        const int tile = blockIdx.x * TRK_WAVES + wave;
        const int ty = tile / a.tx, sx = (tile - ty * a.tx) * TRK_COLS + lane;
        if (tile < a.tiles && sx < a.ws) {                            // a tile or column past the grid adds +0.0
            float T[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = st.pose[i];
            const int px = sx * a.stride;
            for (int r = 0; r < TRK_ROWS; ++r) {
                const int sy = ty * TRK_ROWS + r;
                if (sy < a.hs) R::pixel(ra, T, f, px, sy * a.stride, acc);
            }
        }
#pragma unroll
        for (int k = 0; k < R::BUTTERFLY; ++k)
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) acc[k] += __shfl_xor(acc[k], m, 64);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < SLOTS; ++k) red[wave][k] = acc[k];
        }
        __syncthreads();
        if (threadIdx.x < SLOTS) {
            const int k = threadIdx.x;
            a.partial[(size_t)f * a.partial_stride + (size_t)blockIdx.x * SLOTS + k] =
                (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        }
        __syncthreads();
    }
}

// grid min(n, 65535), 1024 threads: thread (chunk c = t / LANES, slot k = t % LANES), the slots past SLOTS idle; only the
// busy lanes own stack space
template <class R> static __device__ __forceinline__ void track_solve_body(const typename R::Args ra) {
    constexpr int SLOTS = R::SLOTS, CHUNKS = R::CHUNKS, STACK = R::STACK, LANES = 1024 / CHUNKS;
    static_assert(CHUNKS * LANES == 1024 && SLOTS <= LANES, "a chunk's lanes hold a partial's slots");
    static_assert(TRK_MAX_TILES / TRK_WAVES <= CHUNKS * 8 * (1 << (STACK - 1)), "the stack covers every accepted frame");
    const TrackArgs &a = R::common(ra);
    __shared__ double stk[STACK][CHUNKS * SLOTS];
    __shared__ double chunk_sum[CHUNKS][SLOTS];
    __shared__ double S[SLOTS];
    const int t = threadIdx.x, k = t & (LANES - 1), chunk = t >> __builtin_ctz(LANES);
    const int groups = a.groups;
    int padded = 1;
    while (padded < groups) padded <<= 1;
    const int len = padded > CHUNKS ? padded / CHUNKS : 1;            // partials per chunk: a power of two
    for (int f = blockIdx.x; f < a.n; f += gridDim.x) {
        if (a.state[f].done) continue;
        if (k < SLOTS) {
            const double *part = a.partial + (size_t)f * a.partial_stride + k;
            const int first = chunk * len, mine = chunk * SLOTS + k;
            auto at = [&](int i) { return first + i < groups ? part[(size_t)(first + i) * SLOTS] : 0.0; };
            double v;
            if (len >= 8) {
                for (int q = 0; q < len / 8; ++q) {
                    v = ((at(8 * q) + at(8 * q + 1)) + (at(8 * q + 2) + at(8 * q + 3))) +
                        ((at(8 * q + 4) + at(8 * q + 5)) + (at(8 * q + 6) + at(8 * q + 7)));
                    int lvl = 0;
                    for (int j = q; j & 1; j >>= 1) v = stk[lvl++][mine] + v;
                    stk[lvl][mine] = v;
                }
            } else {
                v = len == 4 ? (at(0) + at(1)) + (at(2) + at(3)) : len == 2 ? at(0) + at(1) : at(0);
            }
            chunk_sum[chunk][k] = v;
        }
        __syncthreads();
        if (t < SLOTS) {
            double x[CHUNKS];
#pragma unroll
            for (int i = 0; i < CHUNKS; ++i) x[i] = chunk_sum[i][t];
#pragma unroll
            for (int s = 1; s < CHUNKS; s <<= 1)
#pragma unroll
                for (int i = 0; i < CHUNKS; i += 2 * s) x[i] += x[i + s];
            S[t] = x[0];
        }
        __syncthreads();
        if (t == 0) R::finish(ra, f, S);
        __syncthreads();
    }
}

static_assert(sizeof(TrackState) == 32 * sizeof(int), "track_layout reserves 32 words per triple");

// A rule whose record has no field that depends on the schedule pair
struct TrackSamePerPair {
    template <class A> void operator()(A &, int) const {}
};

// Fills the common record of `ra` (the rule's own fields are the caller's) and enqueues the call: one launch that takes
// the poses in, then two launches per iteration of the schedule.  per_pair(ra, p) sets the rule's fields that belong to
// pair p of the schedule, before that pair's launches take the record by value.
template <class R, class PerPair = TrackSamePerPair>
void track_launch(const TrackCall &c, typename R::Args &ra, void (*begin)(typename R::Args),
                  void (*accum)(typename R::Args), void (*solve)(typename R::Args), hipStream_t s,
                  PerPair per_pair = PerPair()) {
    const int n = c.n;
    const TrackLayout l = track_layout(n, c.H, c.W, R::SLOTS);
    TrackArgs &a = R::common(ra);
    a.n = n, a.H = c.H, a.W = c.W, a.Hm = c.Hm, a.Wm = c.Wm;
    a.disp = c.disp, a.conf = c.confidence, a.depth = c.model_depth, a.normals = c.model_normals;
    a.c2w = c.model_camera_to_world, a.w2c = c.model_world_to_camera;
    std::memcpy(a.q, c.q, sizeof(a.q));
    std::memcpy(a.qm, c.qm, sizeof(a.qm));
    std::memcpy(a.pm, c.pm, sizeof(a.pm));
    a.min_conf = c.min_confidence, a.zmin = c.zmin, a.zmax = c.zmax, a.invalid = c.invalid;
    a.maxd2 = c.max_distance * c.max_distance;
    a.stride = 1, a.ws = a.hs = a.tx = a.tiles = a.groups = 0;
    a.min_inliers = c.min_inliers, a.min_pivot = (double)c.min_pivot;
    a.rot_eps2 = c.rot_eps * c.rot_eps, a.trans_eps2 = c.trans_eps * c.trans_eps;
    a.pose_in = c.pose_in, a.pose_out = c.pose_out, a.rms = c.rms, a.info = c.info, a.sums = c.normal_equations;
    a.state = ws_at<TrackState>(c.workspace, l.state), a.partial = ws_at<double>(c.workspace, l.partial);
    a.partial_stride = (size_t)l.groups * R::SLOTS;
    const unsigned triples = (unsigned)(n < 65535 ? n : 65535);
    hipLaunchKernelGGL(begin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ra);
    for (int p = 0; p < c.pairs; ++p) {
        const TrackGrid g = track_grid(c.H, c.W, c.schedule[2 * p]);
        a.stride = c.schedule[2 * p], a.ws = g.ws, a.hs = g.hs, a.tx = g.tx, a.tiles = g.tiles, a.groups = g.groups;
        per_pair(ra, p);
        for (int it = 0; it < c.schedule[2 * p + 1]; ++it) {
            hipLaunchKernelGGL(accum, dim3((unsigned)g.groups, triples), dim3(256), 0, s, ra);
            hipLaunchKernelGGL(solve, dim3(triples), dim3(1024), 0, s, ra);
        }
    }
}

}  // namespace smx
