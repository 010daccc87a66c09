// k_remap.h -- bilinear remap with the integer rule of include/stereo_mi355x.h (smx_remap_pairs): rectification of raw
// stereo frames through a precomputed map of 1/32-pixel coordinates.
//
// One launch covers both views of n pairs.  A block is a tile of REMAP_TX * REMAP_PX output pixels by REMAP_TY rows of
// one view; each thread owns REMAP_PX adjacent pixels of one row.  The thread reads the map once for its pixels, keeps
// the taps (two clamped row offsets, two clamped columns, the fractions and the inside flags) in registers and applies
// them to every channel of up to `ipt` images (blockIdx.z = view * chunks + chunk).  Every load goes through clamped
// coordinates, so no map value can address outside the input; the constant border replaces a tap outside the input by
// the border value afterwards (a select, no branch).  The texture sampler is not used: its filter weights are not exact.
#pragma once
#include "smx_common.h"

namespace smx {

constexpr int REMAP_TX = 64;     // threads per row of the tile
constexpr int REMAP_TY = 4;      // rows per tile
constexpr int REMAP_PX = 4;      // adjacent output pixels per thread (a dword of uint8 or a float4 of float32)
constexpr int REMAP_IPT = 4;     // images per thread (the taps are reused across them)

struct RemapParams {
    const void *in[2];           // [n][C][Hi][Wi] per view
    const int32_t *map[2];       // [Ho][Wo][2] per view, (x, y) in 1/32 pixel
    void *out[2];                // [n][C][Ho][Wo] per view
    int n, C, Hi, Wi, Ho, Wo;
    int ipt, chunks;             // images per thread, image chunks per view (chunks * ipt >= n)
    int bval_i;                  // uint8 border value
    float bval_f;                // float32 border value
};

// taps of one output pixel
struct RemapTap {
    int r0, r1;                  // clamped row offsets y0 * Wi, (y0 + 1) * Wi
    int c0, c1;                  // clamped columns x0, x0 + 1
    int fx, fy;                  // fractions 0..31
    unsigned in;                 // bit k set: tap k (00, 01, 10, 11) lies inside the input
};

__device__ __forceinline__ RemapTap remap_tap(int qx, int qy, int Hi, int Wi) {
    RemapTap t;
    const int x0 = qx >> 5, y0 = qy >> 5;          // arithmetic shifts: floor; x0 + 1 <= 2^26, no overflow
    t.fx = qx & 31;
    t.fy = qy & 31;
    const int x1 = x0 + 1, y1 = y0 + 1;
    const bool ix0 = x0 >= 0 && x0 < Wi, ix1 = x1 >= 0 && x1 < Wi;
    const bool iy0 = y0 >= 0 && y0 < Hi, iy1 = y1 >= 0 && y1 < Hi;
    t.in = (unsigned)(iy0 && ix0) | (unsigned)(iy0 && ix1) << 1 | (unsigned)(iy1 && ix0) << 2 | (unsigned)(iy1 && ix1) << 3;
    t.c0 = min(max(x0, 0), Wi - 1);
    t.c1 = min(max(x1, 0), Wi - 1);
    t.r0 = min(max(y0, 0), Hi - 1) * Wi;
    t.r1 = min(max(y1, 0), Hi - 1) * Wi;
    return t;
}

// REPLICATE: the clamped taps are the rule; CONSTANT: a tap outside reads the border value
template <bool REPLICATE>
__device__ __forceinline__ uint8_t remap_px(const uint8_t *__restrict__ src, const RemapTap &t, int bval) {
    int p00 = src[t.r0 + t.c0], p01 = src[t.r0 + t.c1], p10 = src[t.r1 + t.c0], p11 = src[t.r1 + t.c1];
    if (!REPLICATE) {
        p00 = (t.in & 1) ? p00 : bval;
        p01 = (t.in & 2) ? p01 : bval;
        p10 = (t.in & 4) ? p10 : bval;
        p11 = (t.in & 8) ? p11 : bval;
    }
    const int gx = 32 - t.fx, gy = 32 - t.fy;
    const int s = gx * gy * p00 + t.fx * gy * p01 + gx * t.fy * p10 + t.fx * t.fy * p11;
    return (uint8_t)((s + 512) >> 10);
}

template <bool REPLICATE>
__device__ __forceinline__ float remap_px(const float *__restrict__ src, const RemapTap &t, float bval) {
    float p00 = src[t.r0 + t.c0], p01 = src[t.r0 + t.c1], p10 = src[t.r1 + t.c0], p11 = src[t.r1 + t.c1];
    if (!REPLICATE) {
        p00 = (t.in & 1) ? p00 : bval;
        p01 = (t.in & 2) ? p01 : bval;
        p10 = (t.in & 4) ? p10 : bval;
        p11 = (t.in & 8) ? p11 : bval;
    }
    const int gx = 32 - t.fx, gy = 32 - t.fy;
    const int w00 = gx * gy, w01 = t.fx * gy, w10 = gx * t.fy, w11 = t.fx * t.fy;
    // a zero weight contributes +0.0 whatever its tap holds (inf or NaN behind it does not leak); -ffp-contract=off
    const float a00 = w00 ? (float)w00 * p00 : 0.0f, a01 = w01 ? (float)w01 * p01 : 0.0f;
    const float a10 = w10 ? (float)w10 * p10 : 0.0f, a11 = w11 ? (float)w11 * p11 : 0.0f;
    const float r = ((a00 + a01) + (a10 + a11)) * 0.0009765625f;
    return r != r ? __uint_as_float(0x7FC00000u) : r;    // every NaN result is the canonical quiet NaN
}

// ---- stores of the VEC form.  A wave is one row segment of 256 output pixels (blockDim = 64 x 4), lane l computing the
// pixels x .. x+3 (x = 4 * global thread column).  Within one plane the row's misalignment s (in elements, 0..3) is the
// same for the whole wave, so lane l stores the ALIGNED group of 4 elements that starts at pixel x - s: elements 0..s-1
// come from lane l-1 (one cross-lane shift), s..3 from itself.  A group with an element outside the row, or whose first
// elements belong to the previous wave (lane 0 when s > 0), is stored element by element; lane 63 also stores its last s
// elements, which fall into the next wave's first group.  Every row width thus gets dword (uint8) or float4 (float32)
// stores everywhere but at the two ends of a wave's segment.

// uint8: the four values packed in a dword, byte k = pixel x + k
__device__ __forceinline__ void remap_store_row(uint8_t *row, int x, int x_wave, int Wo, const uint8_t (&v)[REMAP_PX],
                                                int lane) {
    const uint32_t packed = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    const uint32_t prev = (uint32_t)__shfl_up((int)packed, 1, 64);
    const int s = (int)((uintptr_t)(row + x) & 3);         // wave-uniform
    const uint32_t group = s ? (packed << (8 * s)) | (prev >> (32 - 8 * s)) : packed;
    const int g0 = x - s;                                   // first pixel of this lane's aligned group
    if (g0 >= x_wave && g0 + 3 < Wo) {
        *(uint32_t *)(row + g0) = group;
    } else {
#pragma unroll
        for (int k = 0; k < REMAP_PX; ++k)
            if (g0 + k >= x_wave && g0 + k < Wo) row[g0 + k] = (uint8_t)(group >> (8 * k));
    }
    if (lane == 63 && s) {                                  // the tail that belongs to the next wave's first group
#pragma unroll
        for (int k = 0; k < REMAP_PX; ++k)
            if (k >= REMAP_PX - s && x + k < Wo) row[x + k] = v[k];
    }
}

// float32: the four values shifted by s through a wave-uniform switch (constant register indices, no scratch)
__device__ __forceinline__ void remap_store_row(float *row, int x, int x_wave, int Wo, const float (&v)[REMAP_PX],
                                                int lane) {
    float pv[REMAP_PX];
#pragma unroll
    for (int k = 0; k < REMAP_PX; ++k) pv[k] = __shfl_up(v[k], 1, 64);
    const int s = (int)(((uintptr_t)(row + x) >> 2) & 3);  // wave-uniform (the outputs are 4-byte aligned)
    float g[REMAP_PX];
    switch (s) {
        case 0: g[0] = v[0], g[1] = v[1], g[2] = v[2], g[3] = v[3]; break;
        case 1: g[0] = pv[3], g[1] = v[0], g[2] = v[1], g[3] = v[2]; break;
        case 2: g[0] = pv[2], g[1] = pv[3], g[2] = v[0], g[3] = v[1]; break;
        default: g[0] = pv[1], g[1] = pv[2], g[2] = pv[3], g[3] = v[0]; break;
    }
    const int g0 = x - s;
    if (g0 >= x_wave && g0 + 3 < Wo) {
        *(float4 *)(row + g0) = make_float4(g[0], g[1], g[2], g[3]);
    } else {
#pragma unroll
        for (int k = 0; k < REMAP_PX; ++k)
            if (g0 + k >= x_wave && g0 + k < Wo) row[g0 + k] = g[k];
    }
    if (lane == 63 && s) {
#pragma unroll
        for (int k = 0; k < REMAP_PX; ++k)
            if (k >= REMAP_PX - s && x + k < Wo) row[x + k] = v[k];
    }
}

// VEC: the maps 8-byte and the outputs sizeof(T)-byte aligned (checked on the host), any Wo: the map is read as two
// int4 (rows whose map is 16-byte aligned) or four int2, and the stores are the aligned groups above.  Otherwise every
// pixel is read and stored on its own.
template <typename T, bool REPLICATE, bool VEC>
__global__ __launch_bounds__(REMAP_TX * REMAP_TY) void k_remap(RemapParams p) {
    const int view = blockIdx.z / p.chunks, chunk = blockIdx.z - view * p.chunks;
    const int y = blockIdx.y * REMAP_TY + threadIdx.y;
    const int x_wave = blockIdx.x * REMAP_TX * REMAP_PX;
    const int x = x_wave + threadIdx.x * REMAP_PX;
    if (y >= p.Ho) return;                                  // wave-uniform: a wave is one row
    if (!VEC && x >= p.Wo) return;                          // the VEC stores need every lane of the wave
    const int npx = max(0, min(REMAP_PX, p.Wo - x));
    const int32_t *map = p.map[view] + ((size_t)y * p.Wo + x) * 2;
    RemapTap tap[REMAP_PX];
    if (VEC && npx == REMAP_PX) {
        int q[2 * REMAP_PX];
        if (((uintptr_t)map & 15) == 0) {
            const int4 a = *(const int4 *)map, b = *(const int4 *)(map + 4);
            q[0] = a.x, q[1] = a.y, q[2] = a.z, q[3] = a.w, q[4] = b.x, q[5] = b.y, q[6] = b.z, q[7] = b.w;
        } else {
#pragma unroll
            for (int k = 0; k < REMAP_PX; ++k) {
                const int2 e = *(const int2 *)(map + 2 * k);
                q[2 * k] = e.x, q[2 * k + 1] = e.y;
            }
        }
#pragma unroll
        for (int k = 0; k < REMAP_PX; ++k) tap[k] = remap_tap(q[2 * k], q[2 * k + 1], p.Hi, p.Wi);
    } else {
#pragma unroll
        for (int k = 0; k < REMAP_PX; ++k)
            tap[k] = remap_tap(k < npx ? map[2 * k] : 0, k < npx ? map[2 * k + 1] : 0, p.Hi, p.Wi);
    }
    const T *in = (const T *)p.in[view];
    T *out = (T *)p.out[view];
    const size_t in_plane = (size_t)p.Hi * p.Wi, out_plane = (size_t)p.Ho * p.Wo;
    const size_t out_row = (size_t)y * p.Wo;
    const long long i_end = min((long long)p.n, (long long)(chunk + 1) * p.ipt);
    for (long long plane = (long long)chunk * p.ipt * p.C, pend = i_end * p.C; plane < pend; ++plane) {
        const T *src = in + (size_t)plane * in_plane;
        T *row = out + (size_t)plane * out_plane + out_row;
        T v[REMAP_PX];
#pragma unroll
        for (int k = 0; k < REMAP_PX; ++k) {
            if constexpr (sizeof(T) == 1) v[k] = remap_px<REPLICATE>(src, tap[k], p.bval_i);
            else v[k] = remap_px<REPLICATE>(src, tap[k], p.bval_f);
        }
        if (VEC) {
            remap_store_row(row, x, x_wave, p.Wo, v, (int)threadIdx.x);
        } else {
#pragma unroll
            for (int k = 0; k < REMAP_PX; ++k)
                if (k < npx) row[x + k] = v[k];
        }
    }
}

}  // namespace smx
