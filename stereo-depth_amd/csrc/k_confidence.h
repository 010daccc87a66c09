// k_confidence.h -- per-pixel confidence of a disparity map (include/stereo_mi355x.h: smx_confidence_map).
//
// One launch for the n maps.  A workgroup of CONF_THREADS threads owns a CONF_TW x CONF_TH output tile of one map:
//   1. With a guide, it stages the guide tile plus an R-wide halo (coordinates clamped into the image) in LDS, then runs
//      a separable min / max: every staged row's horizontal (2R+1)-window first (into two more LDS planes), then each
//      output pixel's vertical window over those.  A NaN enters the max as -inf and the min as +inf, so only non-NaN
//      values count, and a window with none is left with max < min.
//   2. Each lane owns one column of the tile and CONF_TH / (CONF_THREADS / CONF_TW) of its rows: D_L is read and conf is
//      written coalesced, a row segment per wave; D_R is gathered from the same row at Y - t, nearly coalesced because t
//      varies slowly along a row.
// Max and min do not depend on the order of evaluation, and every other operation is one float32 round-to-nearest
// (explicit __f*_rn, -ffp-contract=off, the correctly rounded division), so the result does not depend on the split.
#pragma once
#include "smx_common.h"

namespace smx {

constexpr int CONF_TW = 64;                       // tile columns: one per lane
constexpr int CONF_TH = 16;                       // tile rows
constexpr int CONF_THREADS = 256;
constexpr int CONF_ROWS_PER_PASS = CONF_THREADS / CONF_TW;
constexpr int CONF_MAX_RADIUS = 15;
static_assert(CONF_TW == 64 && CONF_TH % CONF_ROWS_PER_PASS == 0, "k_confidence: one wave per tile row segment");

struct ConfArgs {
    const float *left, *right, *guide;            // right, guide: NULL for no LR / texture term
    float *out;
    int n, H, W, radius, tiles_x;
    float lr_scale, texture_scale, invalid;
};

// LDS floats of one workgroup for radius R (host and device): the staged guide (TH + 2R) x (TW + 2R), then the
// horizontal maxima and minima, (TH + 2R) x TW each.
__host__ __device__ constexpr int conf_lds_floats(int R) {
    return (CONF_TH + 2 * R) * (CONF_TW + 2 * R) + 2 * (CONF_TH + 2 * R) * CONF_TW;
}

__device__ __forceinline__ bool conf_valid(float d, float invalid) { return __builtin_isfinite(d) && d != invalid; }

__global__ __launch_bounds__(CONF_THREADS) void k_confidence(ConfArgs a) {
    extern __shared__ float lds[];
    const int R = a.radius;
    const int GW = CONF_TW + 2 * R, GH = CONF_TH + 2 * R;
    float *g = lds;                               // [GH][GW]
    float *hmax = g + GH * GW;                    // [GH][TW]
    float *hmin = hmax + GH * CONF_TW;            // [GH][TW]
    const size_t HW = (size_t)a.H * a.W;
    const int x0 = (blockIdx.x / a.tiles_x) * CONF_TH, y0 = (blockIdx.x % a.tiles_x) * CONF_TW;   // row, column
    const int lane = threadIdx.x % CONF_TW, wrow = threadIdx.x / CONF_TW;
    const int Y = y0 + lane;
    for (int m = blockIdx.y; m < a.n; m += gridDim.y) {
        const size_t base = (size_t)m * HW;
        if (a.guide) {
            __syncthreads();                      // the previous map's planes are read
            const float *gm = a.guide + base;
            for (int r = wrow; r < GH; r += CONF_ROWS_PER_PASS) {
                const float *src = gm + (size_t)min(max(x0 + r - R, 0), a.H - 1) * a.W;
                for (int c = lane; c < GW; c += CONF_TW) g[r * GW + c] = src[min(max(y0 + c - R, 0), a.W - 1)];
            }
            __syncthreads();
            for (int r = wrow; r < GH; r += CONF_ROWS_PER_PASS) {
                const float *row = g + r * GW + lane;
                float mx = -INFINITY, mn = INFINITY;
                for (int j = 0; j <= 2 * R; ++j) {
                    const float v = row[j];
                    const bool nan = __builtin_isnan(v);
                    mx = fmaxf(mx, nan ? -INFINITY : v);
                    mn = fminf(mn, nan ? INFINITY : v);
                }
                hmax[r * CONF_TW + lane] = mx;
                hmin[r * CONF_TW + lane] = mn;
            }
            __syncthreads();
        }
        if (Y >= a.W) continue;                   // no barrier below: whole lanes may leave
#pragma unroll
        for (int i = 0; i < CONF_TH / CONF_ROWS_PER_PASS; ++i) {
            const int r = wrow + i * CONF_ROWS_PER_PASS;
            const int X = x0 + r;
            if (X >= a.H) break;
            const size_t p = base + (size_t)X * a.W + Y;
            const float d = a.left[p];
            float conf = 0.0f;
            if (conf_valid(d, a.invalid)) {
                float c_lr = 1.0f;
                bool ok = true;
                if (a.right) {
                    const float t = floorf(__fadd_rn(d, 0.5f));
                    if (t >= 0.0f && t <= (float)Y) {
                        const float rv = a.right[p - (int)t];
                        if (conf_valid(rv, a.invalid)) {
                            const float e = fabsf(__fsub_rn(d, rv));
                            c_lr = fmaxf(0.0f, __fsub_rn(1.0f, __fdiv_rn(e, a.lr_scale)));
                        } else {
                            ok = false;
                        }
                    } else {
                        ok = false;
                    }
                }
                float c_tex = 1.0f;
                if (a.guide) {
                    float mx = -INFINITY, mn = INFINITY;
                    for (int j = 0; j <= 2 * R; ++j) {
                        mx = fmaxf(mx, hmax[(r + j) * CONF_TW + lane]);
                        mn = fminf(mn, hmin[(r + j) * CONF_TW + lane]);
                    }
                    float range = __fsub_rn(mx, mn);
                    if (!(mx >= mn) || __builtin_isnan(range)) {          // every value NaN, or inf - inf
                        c_tex = 0.0f;
                    } else {
                        if (range == 0.0f) range = 0.0f;                  // -0.0 - +0.0: a zero range is +0.0
                        c_tex = fminf(1.0f, __fdiv_rn(range, a.texture_scale));
                    }
                }
                if (ok) conf = __fmul_rn(c_lr, c_tex);
            }
            a.out[p] = conf;
        }
    }
}

}  // namespace smx
