// k_pyramid.h -- intensity pyramids (smx_intensity_pyramid): level 0, the plane with the pixels that have no surface
// turned into NaNs, and Burt and Adelson's reduce from one level to the next.  The rule, tap by tap, is
// k_track_pyramid_rule.h's pyr_reduce_pixel; tests/track_pyramid_ref.py restates it in NumPy.
//
// Reduce: a workgroup of four waves owns a tile of PYR_TW x PYR_TH output pixels of one plane.  It stages the
// (2 PYR_TW + 3) x (2 PYR_TH + 3) input pixels under the tile's footprints in LDS once, indices clamped to the plane, runs
// the horizontal pass from LDS into LDS for every staged row, and the vertical pass from LDS to the output: the input is
// read once (a halo of 12 % of it twice, by the neighbouring tiles) and nothing but the output is written.
//
// LDS.  A b32 access is served per half wave of 32 lanes over 32 banks.  The horizontal pass reads five taps at a lane
// stride of two pixels, which in a plain row would put lanes l and l + 16 on one bank, so a staged row keeps its even
// columns and its odd columns apart: the taps of output column x are even[x], even[x + 1], even[x + 2] and odd[x],
// odd[x + 1], each read at a lane stride of one word.  The odd part starts PYR_EVEN = 80 = 16 (mod 32) words after the even
// part and a row is PYR_ROW = 160 = 0 (mod 32) words, so the 32 consecutive input pixels that a half wave stages -- it
// walks rows of 160 places of which the first 2 PYR_TW + 3 are pixels, so it never straddles two rows -- go to 16
// consecutive banks from the even part and the other 16 from the odd part.  In both passes a wave is one row of 64
// consecutive output columns, so the horizontal pass's stores and the vertical pass's loads are one word per lane at
// a lane stride of one.  By that bank rule no access of the kernel has a conflict; this is derived from the rule, not
// measured with the conflict counter.
#pragma once
#include "k_track_pyramid_rule.h"
#include "smx_launch.h"

namespace smx {

constexpr int PYR_TW = 64, PYR_TH = 16;                              // a workgroup's output tile: a wave per row, four rows a pass
constexpr int PYR_IN_W = 2 * PYR_TW + 3, PYR_IN_H = 2 * PYR_TH + 3;  // the input pixels under it
constexpr int PYR_EVEN = 80, PYR_ROW = 160;                          // words of a staged row's even part, and of the row
constexpr int PYR_STAGE = (PYR_IN_H * PYR_ROW + 255) / 256;           // places of the staged tile per thread
static_assert(PYR_EVEN >= PYR_TW + 2 && PYR_ROW - PYR_EVEN >= PYR_TW + 1 && PYR_ROW >= PYR_IN_W, "a staged row holds the tile's columns");
static_assert(PYR_EVEN % 32 == 16 && PYR_ROW % 32 == 0, "the bank rule above");

// Level 0: out = plane, NaN where mask (may be NULL) is not finite and > 0; grid-stride, one thread per pixel
__global__ __launch_bounds__(256) void k_pyramid_base(const float *__restrict__ plane, const float *__restrict__ mask,
                                                      float *__restrict__ out, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        float v = plane[i];
        if (mask) {
            const float z = mask[i];
            if (!(std::isfinite(z) && z > 0.0f)) v = __builtin_nanf("");
        }
        out[i] = v;
    }
}

// in: [n][H][W]; out: [n][Ho][Wo], Ho = ceil(H / 2), Wo = ceil(W / 2); grid (ceil(Wo / PYR_TW), ceil(Ho / PYR_TH),
// min(n, 65535)), 256 threads
__global__ __launch_bounds__(256) void k_pyramid_reduce(const float *__restrict__ in, float *__restrict__ out, int n, int H,
                                                        int W, int Ho, int Wo) {
    __shared__ float tile[PYR_IN_H][PYR_ROW];
    __shared__ float hpass[PYR_IN_H][PYR_TW];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int ox = blockIdx.x * PYR_TW, oy = blockIdx.y * PYR_TH;    // the tile's first output pixel
    const int ix = 2 * ox - 2, iy = 2 * oy - 2;                      // the first input pixel under it: an even column
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const float *src = in + (size_t)f * H * W;
        // every load of the thread is issued before the first value is stored: one memory latency per tile, not one
        // per place
        float v[PYR_STAGE];
#pragma unroll
        for (int k = 0; k < PYR_STAGE; ++k) {
            const int idx = t + 256 * k, r = idx / PYR_ROW, j = idx - r * PYR_ROW;
            v[k] = r < PYR_IN_H && j < PYR_IN_W ? src[(size_t)pyr_clamp(iy + r, H) * W + pyr_clamp(ix + j, W)] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < PYR_STAGE; ++k) {
            const int idx = t + 256 * k, r = idx / PYR_ROW, j = idx - r * PYR_ROW;
            if (r < PYR_IN_H && j < PYR_IN_W) tile[r][(j & 1) * PYR_EVEN + (j >> 1)] = v[k];
        }
        __syncthreads();
        for (int idx = t; idx < PYR_IN_H * PYR_TW; idx += 256) {     // a wave per staged row
            const int r = idx >> 6, x = idx & 63;
            const float *even = tile[r], *odd = tile[r] + PYR_EVEN;
            hpass[r][x] = pyr_taps(even[x], odd[x], even[x + 1], odd[x + 1], even[x + 2]);
        }
        __syncthreads();
        if (ox + lane < Wo) {
            float *dst = out + (size_t)f * Ho * Wo;
            for (int y = wave; y < PYR_TH && oy + y < Ho; y += 4)
                dst[(size_t)(oy + y) * Wo + ox + lane] = pyr_taps(hpass[2 * y][lane], hpass[2 * y + 1][lane], hpass[2 * y + 2][lane],
                                                                  hpass[2 * y + 3][lane], hpass[2 * y + 4][lane]);
        }
        // no barrier here: the next plane's staging writes only `tile`, whose readers all passed the second barrier, and
        // `hpass` is written again only behind the next plane's first barrier, which no wave reaches before it has
        // finished reading `hpass` above
    }
}

}  // namespace smx
