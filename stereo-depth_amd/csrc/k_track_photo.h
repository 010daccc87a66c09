// k_track_photo.h -- camera tracking with a photometric term summed into the geometric system
// (smx_track_camera_photometric), and the intensity planes it reads (smx_intensity_planes).  The rule, bit for bit, is
// in include/stereo_mi355x.h; k_track_photo_rule.h holds its per-pixel terms as host/device code, and
// tests/track_photo_ref.py restates it in NumPy.
//
// The launches are k_track.h's with TRKP_SLOTS sums per pixel instead of TRK_SLOTS.  k_track_photo_accum: one wave per
// tile of 64 x TRK_ROWS selected pixels, one lane per column with the sums in registers, an xor butterfly over the 64
// columns, the four tiles of a workgroup through LDS as (t0 + t1) + (t2 + t3).  k_track_photo_solve: one workgroup per
// triple finishes the tile tree.  34 slots do not fit k_track_solve's 32 x 32 threads, so a wave is a chunk here: thread
// (chunk = t / 64, slot = t % 64) of 16 chunks, the lanes past TRKP_SLOTS idle, and a wave reads TRKP_SLOTS consecutive
// doubles of a partial at a time.  A chunk is a power of two of consecutive partials, so chunk trees followed by the
// chunks' tree are the header's adjacent-pairs tree whatever the number of chunks.  No atomics, and nothing passes between
// workgroups inside a launch.
#pragma once
#include "k_track_photo_rule.h"

namespace smx {

// one thread per triple: state and the outputs of "no iteration ran"
__global__ __launch_bounds__(256) void k_track_photo_begin(const TrackPhotoArgs a) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f < a.g.n) trkp_begin(a, f);
}

// grid (groups, min(n, 65535)); wave w of workgroup b owns tile 4 b + w of the selected grid, in row-major order
__global__ __launch_bounds__(256) void k_track_photo_accum(const TrackPhotoArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double red[TRK_WAVES][TRKP_SLOTS];
    for (int f = blockIdx.y; f < a.g.n; f += gridDim.y) {
        const TrackState &st = a.g.state[f];
        if (st.done) continue;                                        // the same for the whole workgroup
        double acc[TRKP_SLOTS];
#pragma unroll
        for (int k = 0; k < TRKP_SLOTS; ++k) acc[k] = 0.0;
        const int tile = blockIdx.x * TRK_WAVES + wave;
        const int ty = tile / a.g.tx, sx = (tile - ty * a.g.tx) * TRK_COLS + lane;
        if (tile < a.g.tiles && sx < a.g.ws) {                        // a tile or column past the grid adds +0.0
            float T[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) T[i] = st.pose[i];
            const int px = sx * a.g.stride;
            for (int r = 0; r < TRK_ROWS; ++r) {
                const int sy = ty * TRK_ROWS + r;
                if (sy < a.g.hs) trkp_pixel(a, T, f, px, sy * a.g.stride, acc);
            }
        }
#pragma unroll
        for (int k = 0; k < TRKP_SLOTS; ++k)
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) acc[k] += __shfl_xor(acc[k], m, 64);
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < TRKP_SLOTS; ++k) red[wave][k] = acc[k];
        }
        __syncthreads();
        if (threadIdx.x < TRKP_SLOTS) {
            const int k = threadIdx.x;
            a.partial[(size_t)f * a.partial_stride + (size_t)blockIdx.x * TRKP_SLOTS + k] =
                (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
        }
        __syncthreads();
    }
}

constexpr int TRKP_CHUNKS = 16;                                       // chunks of consecutive partials per triple: one wave each
constexpr int TRKP_STACK = 7;                                         // levels above a leaf of 8: chunks of up to 512 partials
static_assert(TRK_MAX_TILES / TRK_WAVES <= TRKP_CHUNKS * 8 * (1 << (TRKP_STACK - 1)), "the stack covers every accepted frame");

// grid min(n, 65535), 1024 threads: thread (chunk c = t / 64, slot k = t % 64), the slots past TRKP_SLOTS idle
__global__ __launch_bounds__(1024) void k_track_photo_solve(const TrackPhotoArgs a) {
    __shared__ double stk[TRKP_STACK][TRKP_CHUNKS * TRKP_SLOTS];
    __shared__ double chunk_sum[TRKP_CHUNKS][TRKP_SLOTS];
    __shared__ double S[TRKP_SLOTS];
    const int t = threadIdx.x, k = t & 63, chunk = t >> 6;
    const int groups = a.g.groups;
    int padded = 1;
    while (padded < groups) padded <<= 1;
    const int len = padded > TRKP_CHUNKS ? padded / TRKP_CHUNKS : 1;  // partials per chunk: a power of two
    for (int f = blockIdx.x; f < a.g.n; f += gridDim.x) {
        if (a.g.state[f].done) continue;
        if (k < TRKP_SLOTS) {
            const double *part = a.partial + (size_t)f * a.partial_stride + k;
            const int first = chunk * len, mine = chunk * TRKP_SLOTS + k;
            auto at = [&](int i) { return first + i < groups ? part[(size_t)(first + i) * TRKP_SLOTS] : 0.0; };
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
        if (t < TRKP_SLOTS) {
            double x[TRKP_CHUNKS];
#pragma unroll
            for (int i = 0; i < TRKP_CHUNKS; ++i) x[i] = chunk_sum[i][t];
#pragma unroll
            for (int s = 1; s < TRKP_CHUNKS; s <<= 1)
#pragma unroll
                for (int i = 0; i < TRKP_CHUNKS; i += 2 * s) x[i] += x[i + s];
            S[t] = x[0];
        }
        __syncthreads();
        if (t == 0) trkp_finish(a, f, S);
        __syncthreads();
    }
}

// uint8 [n][C][H][W] -> f32 [n][H][W]: grid-stride over the pixels, one thread per pixel
__global__ __launch_bounds__(256) void k_intensity_planes(const uint8_t *__restrict__ in, float *__restrict__ out, int C,
                                                          size_t plane, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (C == 1) {
            out[i] = (float)in[i];
        } else {
            const size_t f = i / plane;
            const uint8_t *p = in + 2 * f * plane + i;                // frame f's R plane starts at 3 f plane
            const int r = p[0], g = p[plane], b = p[2 * plane];
            out[i] = (float)(77 * r + 150 * g + 29 * b) * 0.00390625f;
        }
    }
}

}  // namespace smx
