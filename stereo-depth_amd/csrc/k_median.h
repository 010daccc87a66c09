// k_median.h -- image-guided weighted median (include/stereo_mi355x.h: smx_weighted_median).
//
// One launch, k_median<SPL>, a grid-stride loop over MED_TH x MED_TW tiles of the n maps (256 pixels, one per thread):
//   1. every thread tests its own pixel for membership of F and copies it from `in` when it is not in F;
//   2. the workgroup compacts its F-pixels into an LDS list (ballot + popcount within a wave, the four wave counts
//      across waves): no workspace and nothing shared between workgroups;
//   3. each wave takes every fourth entry of the list, one F-pixel at a time.  The (2r+1)^2 window offsets are spread
//      over the 64 lanes, SPL per lane (SPL = the smallest instantiated bucket >= (2r+1)^2 / 64, 16 at r = 15); each lane
//      keeps its offsets and spatial weights in registers for the whole launch and, per pixel, its samples as (key,
//      weight) pairs.  T, the smallest and the largest sample key are wave reductions (DPP, __ockl_wfred_*); the median
//      key is then found bit by bit below the highest bit in which those two keys differ, one wave sum per bit.
// The answer is a key, and key -> bits is a bijection, so the output needs no search for the sample that holds it.
// Weights are integers and every sum is exact in uint32, so neither the split over lanes nor the order of a reduction
// can change a result.  out may be holes: holes[p] is read only by the thread that tests p, before any write of a
// median (a barrier lies between), and that thread writes out[p] only in step 1.
#pragma once
#include "smx_common.h"

extern "C" __device__ __attribute__((const)) unsigned int __ockl_wfred_add_u32(unsigned int);
extern "C" __device__ __attribute__((const)) unsigned int __ockl_wfred_min_u32(unsigned int);
extern "C" __device__ __attribute__((const)) unsigned int __ockl_wfred_max_u32(unsigned int);

namespace smx {

constexpr int MED_THREADS = 256;           // 4 waves
constexpr int MED_TH = 8, MED_TW = 32;     // tile: one pixel per thread for the F test
constexpr int MED_MAX_RADIUS = 15;
constexpr int MED_WMAX = 1023;             // largest table value: 961 * 1023^2 < 2^30
static_assert(MED_THREADS == 256, "k_median: one thread per range-table entry and per tile pixel");
static_assert(MED_TH * MED_TW == MED_THREADS, "k_median: one pixel per thread");

// Both tables travel in the kernel arguments (1 KB): the call copies nothing to the device.
struct MedTables {
    uint16_t range[256];
    uint16_t spatial[256];                 // (radius + 1)^2 <= 256 entries used
};

__device__ __forceinline__ bool med_valid(float d, float invalid) { return __builtin_isfinite(d) && d != invalid; }

// The total order of the rule: negative values reversed below positive ones, -0.0 < +0.0.
__device__ __forceinline__ unsigned med_key(float d) {
    const unsigned u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float med_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

template <int SPL>
__global__ __launch_bounds__(MED_THREADS) void k_median(const float *in, const float *holes, const float *guide,
                                                        float *out, int H, int W, int radius, float invalid,
                                                        size_t tiles, int tiles_w, int tiles_per_map, MedTables tab) {
    __shared__ unsigned short rw[256];
    __shared__ unsigned short list[MED_THREADS];
    __shared__ int wcount[MED_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    rw[threadIdx.x] = tab.range[threadIdx.x];
    // this lane's window offsets, for the whole launch (sample s = lane + 64 j, row-major in the window)
    const int side = 2 * radius + 1;
    int ody[SPL], odx[SPL];
    unsigned sw[SPL];
#pragma unroll
    for (int j = 0; j < SPL; ++j) {
        const int s = lane + 64 * j;
        ody[j] = s / side - radius;
        odx[j] = s % side - radius;
        const int at = s < side * side ? abs(ody[j]) * (radius + 1) + abs(odx[j]) : 0;   // < (radius + 1)^2
        sw[j] = s < side * side ? tab.spatial[at] : 0u;
    }
    const size_t HW = (size_t)H * W;
    for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t m = tile / tiles_per_map;
        const int t = (int)(tile - m * tiles_per_map);
        const int x0 = (t / tiles_w) * MED_TH, y0 = (t % tiles_w) * MED_TW;
        const float *inm = in + m * HW, *gm = guide + m * HW;
        float *om = out + m * HW;
        // 1. the F test and the copy of every other pixel
        const int x = x0 + (int)threadIdx.x / MED_TW, y = y0 + (int)threadIdx.x % MED_TW;
        bool f = false;
        if (x < H && y < W) {
            const size_t p = (size_t)x * W + y;
            const float v = inm[p];
            f = holes ? !med_valid(holes[m * HW + p], invalid) : med_valid(v, invalid);
            if (!f) om[p] = v;
        }
        // 2. compaction
        const unsigned long long b = __ballot(f);
        if (lane == 0) wcount[wave] = __popcll(b);
        __syncthreads();                                   // also publishes rw[] on the first tile
        int off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < MED_THREADS / 64; ++w) {
            off += w < wave ? wcount[w] : 0;
            total += wcount[w];
        }
        if (f) list[off + __popcll(b & ((1ull << lane) - 1))] = (unsigned short)threadIdx.x;
        __syncthreads();
        // 3. one wave per F-pixel
        for (int e = wave; e < total; e += MED_THREADS / 64) {
            const int local = list[e];
            const int px = x0 + local / MED_TW, py = y0 + local % MED_TW;
            const float gp = gm[(size_t)px * W + py];
            unsigned key[SPL], wt[SPL];
            unsigned tsum = 0, kmin = 0xFFFFFFFFu, kmax = 0;
#pragma unroll
            for (int j = 0; j < SPL; ++j) {
                const int qx = px + ody[j], qy = py + odx[j];
                unsigned w = 0, k = 0;
                if (sw[j] != 0u && qx >= 0 && qx < H && qy >= 0 && qy < W) {
                    const size_t q = (size_t)qx * W + qy;
                    const float d = inm[q];
                    if (med_valid(d, invalid)) {
                        const float a = fabsf(gp - gm[q]);
                        const int ki = a < 255.0f ? (int)a : 255;          // NaN compares false: 255
                        w = sw[j] * rw[ki];
                        k = med_key(d);
                    }
                }
                key[j] = k;
                wt[j] = w;
                tsum += w;
                if (w != 0u) {
                    kmin = min(kmin, k);
                    kmax = max(kmax, k);
                }
            }
            const unsigned T = __ockl_wfred_add_u32(tsum);
            const size_t p = (size_t)px * W + py;
            if (T == 0u) {                                 // no sample: copied
                if (lane == 0) om[p] = inm[p];
                continue;
            }
            kmin = __ockl_wfred_min_u32(kmin);
            kmax = __ockl_wfred_max_u32(kmax);
            unsigned K = kmin;
            if (kmin != kmax) {
                // the bits above the highest differing bit of kmin and kmax are the answer's; decide the rest
                const int hb = 31 - __clz(kmin ^ kmax);
                K = kmin & ~((2u << hb) - 1u);             // hb = 31: 2u << 31 == 0, the mask clears every bit
                for (int bit = hb; bit >= 0; --bit) {
                    const unsigned probe = K | ((1u << bit) - 1u);   // bit clear, every lower bit set
                    unsigned c = 0;
#pragma unroll
                    for (int j = 0; j < SPL; ++j) c += key[j] <= probe ? wt[j] : 0u;
                    if (2u * __ockl_wfred_add_u32(c) < T) K |= 1u << bit;
                }
            }
            if (lane == 0) om[p] = med_unkey(K);
        }
        __syncthreads();                                   // list[] and wcount[] are reused by the next tile
    }
}

}  // namespace smx
