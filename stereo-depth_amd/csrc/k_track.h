// k_track.h -- frame-to-model camera tracking by projective point-to-plane ICP (smx_track_camera).  The rule, bit for bit,
// is in include/stereo_mi355x.h; k_track_rule.h holds its per-pixel terms and its solve as host/device code, and
// tests/track_ref.py restates it in NumPy.
//
// An iteration is two launches.  k_track_accum: one wave per tile of 64 x TRK_ROWS selected pixels, one lane per column
// walking its rows top to bottom with the thirty float64 sums (and the count of accepted pixels) in registers; the 64
// columns are reduced by an xor butterfly -- lanes l and l^1 first, every lane ending with the same bits as an
// adjacent-pairs tree since a + b = b + a -- and the four tiles of a workgroup through LDS, (t0 + t1) + (t2 + t3), which
// is two levels of the tile tree.  k_track_solve: one workgroup per triple finishes the tile tree over the groups of four
// (thread = (group of consecutive partials, term): a chunk's tree with a stack of one value per level in LDS, then the
// chunks' tree), and its first thread solves the 6 x 6 system, updates the pose and writes the outputs and the stop
// flags.  Both return at once for a triple that has stopped.  No atomics, and nothing passes between workgroups inside
// a launch: what one launch writes the next one reads.
#pragma once
#include "k_track_rule.h"

namespace smx {

// one thread per triple: state and the outputs of "no iteration ran"
__global__ __launch_bounds__(256) void k_track_begin(const TrackArgs a) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < a.n) trk_begin(a, f);
}

// grid (groups, min(n, 65535)); wave w of workgroup b owns tile 4 b + w of the selected grid, in row-major order
__global__ __launch_bounds__(256) void k_track_accum(const TrackArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double red[TRK_WAVES][TRK_SLOTS];
    for (int f = blockIdx.y; f < a.n; f += gridDim.y) {
        const TrackState &st = a.state[f];
        if (st.done) continue;                                        // the same for the whole workgroup
        double acc[TRK_SLOTS];
#pragma unroll
        for (int k = 0; k < TRK_SLOTS; ++k) acc[k] = 0.0;
        const int tile = blockIdx.x * TRK_WAVES + wave;
        const int ty = tile / a.tx, sx = (tile - ty * a.tx) * TRK_COLS + lane;
        if (tile < a.tiles && sx < a.ws) {                            // a tile or column past the grid adds +0.0
            float T[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = st.pose[i];
            const int px = sx * a.stride;
            for (int r = 0; r < TRK_ROWS; ++r) {
                const int sy = ty * TRK_ROWS + r;
                if (sy < a.hs) trk_pixel(a, T, f, px, sy * a.stride, acc);
            }
        }
#pragma unroll
        for (int k = 0; k <= TRK_TERMS; ++k)
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) acc[k] += __shfl_xor(acc[k], m, 64);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < TRK_SLOTS; ++k) red[wave][k] = acc[k];
        }
        __syncthreads();
        if (threadIdx.x < TRK_SLOTS) {
            const int k = threadIdx.x;
            a.partial[(size_t)f * a.partial_stride + (size_t)blockIdx.x * TRK_SLOTS + k] =
                (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        }
        __syncthreads();
    }
}

constexpr int TRK_CHUNKS = 32;                                        // chunks of consecutive partials per triple
constexpr int TRK_STACK = 6;                                          // levels above a leaf of 8: chunks of up to 256 partials
static_assert(TRK_MAX_TILES / TRK_WAVES <= TRK_CHUNKS * 8 * (1 << (TRK_STACK - 1)), "the stack covers every accepted frame");

// grid min(n, 65535), 1024 threads: thread (chunk c = t / 32, term k = t % 32)
__global__ __launch_bounds__(1024) void k_track_solve(const TrackArgs a) {
    __shared__ double stk[TRK_STACK][1024];
    __shared__ double chunk_sum[TRK_CHUNKS][TRK_SLOTS];
    __shared__ double S[TRK_SLOTS];
    const int t = threadIdx.x, k = t & 31, chunk = t >> 5;
    int padded = 1;
    while (padded < a.groups) padded <<= 1;
    const int len = padded > TRK_CHUNKS ? padded / TRK_CHUNKS : 1;    // partials per chunk: a power of two
    for (int f = blockIdx.x; f < a.n; f += gridDim.x) {
        if (a.state[f].done) continue;
        const double *part = a.partial + (size_t)f * a.partial_stride + k;
        const int first = chunk * len;
        auto at = [&](int i) { return first + i < a.groups ? part[(size_t)(first + i) * TRK_SLOTS] : 0.0; };
        double v;
        if (len >= 8) {
            for (int q = 0; q < len / 8; ++q) {
                v = ((at(8 * q) + at(8 * q + 1)) + (at(8 * q + 2) + at(8 * q + 3))) +
                    ((at(8 * q + 4) + at(8 * q + 5)) + (at(8 * q + 6) + at(8 * q + 7)));
                int lvl = 0;
                for (int j = q; j & 1; j >>= 1) v = stk[lvl++][t] + v;
                stk[lvl][t] = v;
            }
        } else {
            v = len == 4 ? (at(0) + at(1)) + (at(2) + at(3)) : len == 2 ? at(0) + at(1) : at(0);
        }
        chunk_sum[chunk][k] = v;
        __syncthreads();
        if (t < TRK_SLOTS) {
            double x[TRK_CHUNKS];
#pragma unroll
            for (int i = 0; i < TRK_CHUNKS; ++i) x[i] = chunk_sum[i][t];
#pragma unroll
            for (int s = 1; s < TRK_CHUNKS; s <<= 1)
#pragma unroll
                for (int i = 0; i < TRK_CHUNKS; i += 2 * s) x[i] += x[i + s];
            S[t] = x[0];
        }
        __syncthreads();
        if (t == 0) trk_finish(a, f, S);
        __syncthreads();
    }
}

}  // namespace smx
