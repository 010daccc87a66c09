// k_temporal.h -- motion-gated temporal filter of disparity-map streams (include/stereo_mi355x.h: smx_temporal_filter).
//
// One launch for the n maps.  A workgroup of TEMP_THREADS threads owns a TEMP_TW x TEMP_TH output tile of one map:
//   1. Each lane owns one column of the tile and TEMP_PIX of its rows.  It issues the loads of its pixels' d, c, D and A
//      first, so that they are in flight while the motion window is staged.
//   2. e = |g - G| over the tile plus an R-wide halo (coordinates clamped into the image) goes to LDS; the interior
//      guide values are copied to guide_out on the way (no second read of g).
//   3. Separable window sum in the order of the rule: every staged row's horizontal sum r(dy) in dx order (into a second
//      LDS plane), then each output pixel's vertical sum over those in dy order.
//   4. The per-pixel update of the rule; out, D' and A' are written coalesced, a row segment per wave.
// State and outputs are read and written at the thread's own pixels only, so out may be disp.  Every operation is one
// float32 round-to-nearest (explicit __f*_rn, -ffp-contract=off, the correctly rounded division), so the result does
// not depend on the split.  No scratch, no allocation, no host synchronisation: the launch can be captured in a graph.
#pragma once
#include "smx_common.h"

namespace smx {

constexpr int TEMP_TW = 64;                       // tile columns: one per lane
constexpr int TEMP_TH = 16;                       // tile rows
constexpr int TEMP_THREADS = 256;
constexpr int TEMP_ROWS_PER_PASS = TEMP_THREADS / TEMP_TW;
constexpr int TEMP_PIX = TEMP_TH / TEMP_ROWS_PER_PASS;   // output pixels per lane
constexpr int TEMP_MAX_RADIUS = 7;
static_assert(TEMP_TW == 64 && TEMP_TH % TEMP_ROWS_PER_PASS == 0, "k_temporal: one wave per tile row segment");

struct TemporalArgs {
    const float *disp, *conf, *guide, *prev;      // conf NULL: every valid measurement weighs 1
    float *state_disp, *state_weight;
    float *guide_out, *out;                       // guide_out NULL: not written
    int n, H, W, radius, tiles_x;
    float threshold, decay, max_diff, max_weight, min_weight, invalid;
};

// LDS floats of one workgroup for radius R (host and device): e over (TH + 2R) x (TW + 2R), then the row sums,
// (TH + 2R) x TW.
__host__ __device__ constexpr int temporal_lds_floats(int R) {
    return (TEMP_TH + 2 * R) * (TEMP_TW + 2 * R) + (TEMP_TH + 2 * R) * TEMP_TW;
}

__device__ __forceinline__ bool temporal_valid(float d, float invalid) {
    return __builtin_isfinite(d) && d != invalid;
}

__global__ __launch_bounds__(TEMP_THREADS) void k_temporal(TemporalArgs a) {
    extern __shared__ float lds[];
    const int R = a.radius, side = 2 * R + 1;
    const int GW = TEMP_TW + 2 * R, GH = TEMP_TH + 2 * R;
    float *e = lds;                               // [GH][GW]
    float *rsum = e + GH * GW;                    // [GH][TW]
    const size_t HW = (size_t)a.H * a.W;
    const int x0 = (blockIdx.x / a.tiles_x) * TEMP_TH, y0 = (blockIdx.x % a.tiles_x) * TEMP_TW;   // row, column
    const int lane = threadIdx.x % TEMP_TW, wrow = threadIdx.x / TEMP_TW;
    const int Y = y0 + lane;
    const float T = __fmul_rn(a.threshold, (float)(side * side));
    for (int m = blockIdx.y; m < a.n; m += gridDim.y) {
        const size_t base = (size_t)m * HW;
        float d[TEMP_PIX], c[TEMP_PIX], D[TEMP_PIX], A[TEMP_PIX];
#pragma unroll
        for (int i = 0; i < TEMP_PIX; ++i) {
            const int X = x0 + wrow + i * TEMP_ROWS_PER_PASS;
            d[i] = c[i] = D[i] = A[i] = 0.0f;
            if (X < a.H && Y < a.W) {
                const size_t p = base + (size_t)X * a.W + Y;
                d[i] = a.disp[p];
                c[i] = a.conf ? a.conf[p] : 1.0f;
                D[i] = a.state_disp[p];
                A[i] = a.state_weight[p];
            }
        }
        __syncthreads();                          // the previous map's planes are read
        const float *gm = a.guide + base, *pm = a.prev + base;
        for (int r = wrow; r < GH; r += TEMP_ROWS_PER_PASS) {
            const int Xs = x0 + r - R;
            const size_t row = (size_t)min(max(Xs, 0), a.H - 1) * a.W;
            const bool copy_row = a.guide_out && r >= R && r < R + TEMP_TH && Xs < a.H;
            for (int cc = lane; cc < GW; cc += TEMP_TW) {
                const int Ys = y0 + cc - R;
                const size_t q = row + min(max(Ys, 0), a.W - 1);
                const float g = gm[q];
                e[r * GW + cc] = fabsf(__fsub_rn(g, pm[q]));
                if (copy_row && cc >= R && cc < R + TEMP_TW && Ys < a.W) a.guide_out[base + q] = g;
            }
        }
        __syncthreads();
        for (int r = wrow; r < GH; r += TEMP_ROWS_PER_PASS) {
            const float *er = e + r * GW + lane;
            float s = er[0];
            for (int j = 1; j < side; ++j) s = __fadd_rn(s, er[j]);
            rsum[r * TEMP_TW + lane] = s;
        }
        __syncthreads();
        if (Y < a.W) {
#pragma unroll
            for (int i = 0; i < TEMP_PIX; ++i) {
                const int r = wrow + i * TEMP_ROWS_PER_PASS;
                const int X = x0 + r;
                if (X >= a.H) break;
                float S = rsum[r * TEMP_TW + lane];
                for (int j = 1; j < side; ++j) S = __fadd_rn(S, rsum[(r + j) * TEMP_TW + lane]);
                const bool still = S <= T;                           // NaN: not static
                const bool dv = temporal_valid(d[i], a.invalid);
                float w = 0.0f;
                if (dv) w = a.conf ? (c[i] > 0.0f ? fminf(c[i], 1.0f) : 0.0f) : 1.0f;
                const float aw = __fmul_rn(A[i], a.decay);
                const bool hist = aw > 0.0f && still && temporal_valid(D[i], a.invalid);
                float o, nA;
                if (dv && hist && fabsf(__fsub_rn(d[i], D[i])) <= a.max_diff) {
                    const float sw = __fadd_rn(aw, w);
                    o = __fdiv_rn(__fadd_rn(__fmul_rn(aw, D[i]), __fmul_rn(w, d[i])), sw);
                    nA = fminf(sw, a.max_weight);
                } else if (dv) {                                     // no history, or disagreement: reset
                    o = d[i];
                    nA = w;
                } else if (hist && aw >= a.min_weight) {             // hold with a decaying weight
                    o = D[i];
                    nA = aw;
                } else {
                    o = a.invalid;
                    nA = 0.0f;
                }
                const size_t p = base + (size_t)X * a.W + Y;
                a.out[p] = o;
                a.state_disp[p] = o;
                a.state_weight[p] = nA;
            }
        }
    }
}

}  // namespace smx
