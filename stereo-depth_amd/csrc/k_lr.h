// k_lr.h -- left-right consistency check (include/stereo_mi355x.h: smx_compute_lr_*, smx_lr_check).
//
// The right-view map is the engine's own left-referenced problem on the mirrored, swapped pair:
// D_R = flip(E(flip R, flip L)).  An LR call of n pairs is ONE engine call of 2n internal pairs -- (L_i, R_i) and
// (flip R_i, flip L_i) -- so the aggregation kernel sees twice the pairs and picks its shape as for any batch.  Two
// kernels surround it:
//   k_lr_pack   writes the packed inputs [L_0 .. L_n-1, flip R_0 .. flip R_n-1] and [R_0 .., flip L_0 ..] in one launch
//               (bandwidth-bound: straight half in 16-byte chunks where the pointers allow, mirrored half reads each row
//               reversed and writes it forwards);
//   k_lr_check  one workgroup per output row: stages the right-view row in LDS (reversed addressing for the mirrored
//               half: no un-flip pass), writes right_out from it, then checks every left pixel against the gathered
//               D_R[X][Y - t] (left-right check).
#pragma once
#include "smx_common.h"

namespace smx {

constexpr int LR_THREADS = 256;            // 4 waves
constexpr int LR_LDS_W = 4096;             // widest row staged in LDS (16 KB); wider rows gather from global memory
constexpr int LR_PACK_ITEMS = 4;           // mirrored half: output elements per thread

// blockIdx.y: 0 = L -> pl (straight), 1 = R -> pr (straight), 2 = R -> pl + half (mirrored), 3 = L -> pr + half (mirrored).
// rows = n * planes * H rows of W elements of T per input; vec: every pointer (and pl / pr + half) is 16-byte aligned.
template <typename T>
__global__ __launch_bounds__(LR_THREADS) void k_lr_pack(const T *__restrict__ L, const T *__restrict__ R, T *__restrict__ pl,
                                                        T *__restrict__ pr, long rows, int W, int vec) {
    const size_t half = (size_t)rows * W;                  // elements per input
    const int which = blockIdx.y;
    const T *src = (which == 0 || which == 3) ? L : R;
    T *dst = (which == 0 || which == 2) ? pl : pr;
    const size_t tid = (size_t)blockIdx.x * LR_THREADS + threadIdx.x, stride = (size_t)gridDim.x * LR_THREADS;
    if (which < 2) {
        constexpr int V = 16 / sizeof(T);
        size_t done = 0;
        if (vec) {
            const size_t chunks = half / V;
            const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
            uint4 *d4 = reinterpret_cast<uint4 *>(dst);
            for (size_t c = tid; c < chunks; c += stride) d4[c] = s4[c];
            done = chunks * V;
        }
        for (size_t i = done + tid; i < half; i += stride) dst[i] = src[i];
        return;
    }
    dst += half;
    const int groups = (W + LR_PACK_ITEMS - 1) / LR_PACK_ITEMS;
    const size_t items = (size_t)rows * groups;
    for (size_t it = tid; it < items; it += stride) {
        const size_t row = it / groups;
        const int y0 = (int)(it - row * groups) * LR_PACK_ITEMS;
        const T *s = src + row * W;
        T *d = dst + row * W;
        T v[LR_PACK_ITEMS];
#pragma unroll
        for (int k = 0; k < LR_PACK_ITEMS; ++k) v[k] = (y0 + k < W) ? s[W - 1 - (y0 + k)] : T(0);
        if (vec && (W % LR_PACK_ITEMS) == 0) {             // row starts stay aligned to 4 elements
            if constexpr (sizeof(T) == 4) {
                *reinterpret_cast<float4 *>(d + y0) = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                *reinterpret_cast<uchar4 *>(d + y0) = make_uchar4(v[0], v[1], v[2], v[3]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < LR_PACK_ITEMS; ++k)
                if (y0 + k < W) d[y0 + k] = v[k];
        }
    }
}

// The rule of include/stereo_mi355x.h (smx_compute_lr_*), float32, no contraction (there is no multiply).
__device__ __forceinline__ bool lr_ok(float dl, int y, const float *dr_row, bool mirrored, int W, float max_diff) {
    const float t = floorf(dl + 0.5f);
    if (!(__builtin_isfinite(t) && t >= 0.0f && t <= (float)y)) return false;
    const int yr = y - (int)t;
    const float dr = dr_row[mirrored ? W - 1 - yr : yr];
    return fabsf(dl - dr) <= max_diff;                     // NaN D_R: false
}

// grid.x = n * H rows.  left / right / out / right_out: [n][H][W].  MIRRORED: `right` holds flip(D_R) (the raw output of
// the mirrored internal pairs).  LDS: the row fits LR_LDS_W.  out may alias left (each element is read, then written, by
// the same thread); right must not alias out.
template <bool MIRRORED, bool LDS>
__global__ __launch_bounds__(LR_THREADS) void k_lr_check(const float *left, const float *__restrict__ right, float *out,
                                                         float *__restrict__ right_out, int W, float max_diff, float invalid,
                                                         int vec) {
    __shared__ float row[LDS ? LR_LDS_W : 1];
    const size_t base = (size_t)blockIdx.x * W;
    const float *rrow = right + base;
    const float *dr = rrow;                                // where lr_ok gathers (global: raw addressing)
    bool mir = MIRRORED;
    if (LDS) {
        for (int y = threadIdx.x; y < W; y += LR_THREADS) {
            const float v = rrow[MIRRORED ? W - 1 - y : y];
            row[y] = v;
            if (right_out) right_out[base + y] = v;
        }
        __syncthreads();
        dr = row;
        mir = false;
    } else if (right_out) {
        for (int y = threadIdx.x; y < W; y += LR_THREADS) right_out[base + y] = rrow[MIRRORED ? W - 1 - y : y];
    }
    const float *lrow = left + base;
    float *orow = out + base;
    if (vec) {                                             // W % 4 == 0 and 16-byte aligned rows: float4 loads / stores
        for (int y0 = threadIdx.x * 4; y0 < W; y0 += LR_THREADS * 4) {
            const float4 l4 = *reinterpret_cast<const float4 *>(lrow + y0);
            float4 o4;
            o4.x = lr_ok(l4.x, y0 + 0, dr, mir, W, max_diff) ? l4.x : invalid;
            o4.y = lr_ok(l4.y, y0 + 1, dr, mir, W, max_diff) ? l4.y : invalid;
            o4.z = lr_ok(l4.z, y0 + 2, dr, mir, W, max_diff) ? l4.z : invalid;
            o4.w = lr_ok(l4.w, y0 + 3, dr, mir, W, max_diff) ? l4.w : invalid;
            *reinterpret_cast<float4 *>(orow + y0) = o4;
        }
    } else {
        for (int y = threadIdx.x; y < W; y += LR_THREADS) {
            const float dl = lrow[y];
            orow[y] = lr_ok(dl, y, dr, mir, W, max_diff) ? dl : invalid;
        }
    }
}

}  // namespace smx
