// k_sgm.h -- semi-global matching (include/stereo_mi355x.h: smx_sgm).
//
// Launches of one call, all on the caller's stream, with the workspace layout of tu_sgm.hip:
//   1. k_sgm_census: both views of the n pairs.  A 64 x 4 tile of gray values with a 4-column and 3-row halo in LDS
//      (coordinates clamped), then one 62-bit census per pixel; the left gray plane is written when asked for.
//   2. k_sgm_paths<DPL>, one launch per axis (horizontal, vertical and, with 8 paths, the two diagonals).  One wave
//      marches one line of the image forward and then backward; lane l owns the DPL disparities l*DPL .. l*DPL+DPL-1.
//      The cost is XOR + popcount of the census on the fly, the neighbours i-1 / i+1 come across lanes by shuffle, and
//      M_r(q) is one wave min reduction per step.  Each pixel lies on exactly one line per axis, so a wave owns its
//      S cells for the whole launch: the first pass of the call stores L_r, every other pass adds L_r to S (u16).
//   3. k_sgm_right_wta<DPL> (LR check on, or the right-view map asked for): iR(y, x') for every right-view pixel, one
//      wave per pixel, and the right-view map f32(dmin + iR) when asked for.
//   4. k_sgm_select<DPL>: winner, uniqueness, LR test and subpixel value, one wave per pixel.
// Every value is an integer until the one float32 division of the subpixel step, so the result does not depend on
// how the work is split.
#pragma once
#include "smx_common.h"

extern "C" __device__ __attribute__((const)) unsigned int __ockl_wfred_min_u32(unsigned int);

namespace smx {

constexpr int SGM_THREADS = 256;                   // 4 waves
constexpr int SGM_TW = 64, SGM_TH = 4;             // census tile: one pixel per thread
constexpr int SGM_RX = 4, SGM_RY = 3;              // census window 9 x 7
constexpr int SGM_LW = SGM_TW + 2 * SGM_RX, SGM_LH = SGM_TH + 2 * SGM_RY;
constexpr unsigned SGM_BIG = 0x4000u;              // a disparity outside 0..D-1: never the min
static_assert(SGM_TW * SGM_TH == SGM_THREADS, "k_sgm_census: one pixel per thread");

enum SgmAxis { SGM_HORIZONTAL = 0, SGM_VERTICAL = 1, SGM_DIAG_DOWN_RIGHT = 2, SGM_DIAG_DOWN_LEFT = 3 };

// The engine's step-1 formula, no contraction (-ffp-contract=off and explicit round-to-nearest operations).
__device__ __forceinline__ float sgm_gray_rgb(float r, float g, float b) {
    return __fadd_rn(__fadd_rn(__fmul_rn(0.2989f, r), __fmul_rn(0.5870f, g)), __fmul_rn(0.1140f, b));
}

// grid: (tiles_x * tiles_y, min(2n, 65535)), a grid-stride loop over the images z in 0..2n-1: z < n is left pair z,
// z >= n right pair z - n.  frames: [n][C][H][W].
__global__ __launch_bounds__(SGM_THREADS) void k_sgm_census(const void *left, const void *right, int C, int f32, int n,
                                                            int H, int W, int tiles_x, uint64_t *cen_l, uint64_t *cen_r,
                                                            float *gray_out) {
    __shared__ float tile[SGM_LH][SGM_LW];
    const size_t HW = (size_t)H * W;
    const int tx0 = (blockIdx.x % tiles_x) * SGM_TW, ty0 = (blockIdx.x / tiles_x) * SGM_TH;
    const int ly = threadIdx.x / SGM_TW, lx = threadIdx.x % SGM_TW;
    const int y = ty0 + ly, x = tx0 + lx;
    for (int z = blockIdx.y; z < 2 * n; z += gridDim.y) {
        const bool is_left = z < n;
        const size_t pair = is_left ? z : z - n;
        const void *src = is_left ? left : right;
        __syncthreads();                                         // the previous image's tile is read
        for (int k = threadIdx.x; k < SGM_LH * SGM_LW; k += SGM_THREADS) {
            const int ty = k / SGM_LW, tx = k % SGM_LW;
            const int gy = min(max(ty0 + ty - SGM_RY, 0), H - 1), gx = min(max(tx0 + tx - SGM_RX, 0), W - 1);
            const size_t at = pair * C * HW + (size_t)gy * W + gx;
            float v;
            if (f32) {
                const float *p = (const float *)src;
                v = C == 1 ? p[at] : sgm_gray_rgb(p[at], p[at + HW], p[at + 2 * HW]);
            } else {
                const uint8_t *p = (const uint8_t *)src;
                v = C == 1 ? (float)p[at] : sgm_gray_rgb((float)p[at], (float)p[at + HW], (float)p[at + 2 * HW]);
            }
            tile[ty][tx] = v;
        }
        __syncthreads();
        if (y >= H || x >= W) continue;
        const float c = tile[ly + SGM_RY][lx + SGM_RX];
        uint64_t bits = 0;
        int k = 0;
#pragma unroll
        for (int dy = -SGM_RY; dy <= SGM_RY; ++dy)
#pragma unroll
            for (int dx = -SGM_RX; dx <= SGM_RX; ++dx) {
                if (dy == 0 && dx == 0) continue;
                bits |= (uint64_t)(tile[ly + SGM_RY + dy][lx + SGM_RX + dx] < c) << k;   // bit k: k-th offset, row-major
                ++k;
            }
        const size_t p = pair * HW + (size_t)y * W + x;
        (is_left ? cen_l : cen_r)[p] = bits;
        if (is_left && gray_out) gray_out[p] = c;
    }
}

// DPL u16 values of one lane, moved as one aligned access (Dp is a multiple of DPL).
template <int DPL> struct SgmVec;
template <> struct SgmVec<1> { using T = uint16_t; };
template <> struct SgmVec<2> { using T = uint32_t; };
template <> struct SgmVec<4> { using T = uint64_t; };

template <int DPL> __device__ __forceinline__ void sgm_unpack(typename SgmVec<DPL>::T v, unsigned (&s)[DPL]) {
#pragma unroll
    for (int k = 0; k < DPL; ++k) s[k] = (unsigned)(v >> (16 * k)) & 0xFFFFu;
}
template <int DPL> __device__ __forceinline__ typename SgmVec<DPL>::T sgm_pack(const unsigned (&s)[DPL]) {
    typename SgmVec<DPL>::T v = 0;
#pragma unroll
    for (int k = 0; k < DPL; ++k) v |= (typename SgmVec<DPL>::T)(s[k] & 0xFFFFu) << (16 * k);
    return v;
}

struct SgmPathArgs {
    const uint64_t *cen_l, *cen_r;
    uint16_t *S;                  // [n][H][W][Dp]
    int n, H, W, dmin, D, Dp, P1, P2;
    int axis, lines;              // lines per pair
    int init;                     // 1: the forward pass stores L_r (the first pass of the call)
};

// The loaded operands of one step: the left census, the right census of each owned disparity, the S vector.
template <int DPL> struct SgmStep {
    uint64_t c;
    uint64_t r[DPL];
    typename SgmVec<DPL>::T s;
};

// One march along a line: start (y0, x0), step (dy, dx), len pixels.  The loads run PF steps ahead of the recurrence
// (double-buffered chunks of PF steps), so a step waits on the min reduction, not on memory.
template <int DPL>
__device__ __forceinline__ void sgm_march(const SgmPathArgs &a, size_t pix0, int y0, int x0, int dy, int dx, int len,
                                          bool store) {
    constexpr int PF = DPL == 4 ? 2 : 4;
    const int lane = threadIdx.x & 63;
    const int i0 = lane * DPL;
    const bool owns = i0 < a.Dp;
    const bool read_s = !store && owns;
    using V = typename SgmVec<DPL>::T;
    const uint64_t *cl = a.cen_l + pix0, *cr = a.cen_r + pix0;
    const V *Sr = (const V *)(a.S + pix0 * a.Dp) + lane;
    V *S = (V *)(a.S + pix0 * a.Dp) + lane;
    const int vpp = a.Dp / DPL;                    // vectors per pixel
    // loads of step min(t, len - 1): past the end they repeat the last pixel and are not used
    auto load = [&](SgmStep<DPL> &st, int t) {
        t = min(t, len - 1);
        const int y = y0 + t * dy, x = x0 + t * dx;
        const size_t px = (size_t)y * a.W + x;
        st.c = cl[px];
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const int xr = x - a.dmin - (i0 + k);
            st.r[k] = (xr >= 0 && i0 + k < a.D) ? cr[px - a.dmin - (i0 + k)] : 0;
        }
        st.s = read_s ? Sr[px * vpp] : (V)0;
    };
    SgmStep<DPL> cur[PF], nxt[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j) load(cur[j], j);
    unsigned Lp[DPL], M = 0;
    for (int t0 = 0; t0 < len; t0 += PF) {
#pragma unroll
        for (int j = 0; j < PF; ++j) load(nxt[j], t0 + PF + j);
#pragma unroll
        for (int j = 0; j < PF; ++j) {
            const int t = t0 + j;
            if (t >= len) break;
            const int xc = x0 + t * dx;
            const size_t px = (size_t)(y0 + t * dy) * a.W + xc;
            unsigned L[DPL];
#pragma unroll
            for (int k = 0; k < DPL; ++k)
                L[k] = (xc - a.dmin - (i0 + k) >= 0) ? (unsigned)__popcll(cur[j].c ^ cur[j].r[k]) : 64u;
            if (t > 0) {
                const unsigned up = __shfl_up(Lp[DPL - 1], 1);       // L(q, i0 - 1) from lane - 1
                const unsigned dn = __shfl_down(Lp[0], 1);           // L(q, i0 + DPL) from lane + 1
                const unsigned mp2 = M + (unsigned)a.P2;
#pragma unroll
                for (int k = 0; k < DPL; ++k) {
                    const unsigned lm = k > 0 ? Lp[k - 1] : (lane > 0 ? up : SGM_BIG);
                    const unsigned lp = k < DPL - 1 ? Lp[k + 1] : (lane < 63 ? dn : SGM_BIG);
                    const unsigned best = min(min(Lp[k], mp2), min(lm, lp) + (unsigned)a.P1);
                    L[k] = L[k] + best - M;
                }
            }
            unsigned lmin = SGM_BIG;
#pragma unroll
            for (int k = 0; k < DPL; ++k) {
                if (i0 + k >= a.D) L[k] = SGM_BIG;
                lmin = min(lmin, L[k]);
            }
            M = __ockl_wfred_min_u32(lmin);
            if (owns) {
                unsigned sv[DPL];
                sgm_unpack<DPL>(cur[j].s, sv);
#pragma unroll
                for (int k = 0; k < DPL; ++k) sv[k] = store ? L[k] : sv[k] + L[k];
                S[px * vpp] = sgm_pack<DPL>(sv);
            }
#pragma unroll
            for (int k = 0; k < DPL; ++k) Lp[k] = L[k];
        }
#pragma unroll
        for (int j = 0; j < PF; ++j) cur[j] = nxt[j];
    }
}

// One wave per (pair, line); the wave marches its line forward, then backward.
template <int DPL>
__global__ __launch_bounds__(SGM_THREADS) void k_sgm_paths(SgmPathArgs a) {
    const size_t w = (size_t)blockIdx.x * (SGM_THREADS / 64) + (threadIdx.x >> 6);
    if (w >= (size_t)a.n * a.lines) return;                      // whole waves only
    const int pair = (int)(w / a.lines), j = (int)(w % a.lines);
    const size_t pix0 = (size_t)pair * a.H * a.W;
    int y0, x0, dy, dx, len;
    if (a.axis == SGM_HORIZONTAL) {
        y0 = j, x0 = 0, dy = 0, dx = 1, len = a.W;
    } else if (a.axis == SGM_VERTICAL) {
        y0 = 0, x0 = j, dy = 1, dx = 0, len = a.H;
    } else if (a.axis == SGM_DIAG_DOWN_RIGHT) {                  // lines x - y = const
        if (j < a.W) y0 = 0, x0 = j;
        else y0 = j - a.W + 1, x0 = 0;
        dy = 1, dx = 1, len = min(a.H - y0, a.W - x0);
    } else {                                                     // lines x + y = const
        if (j < a.W) y0 = 0, x0 = j;
        else y0 = j - a.W + 1, x0 = a.W - 1;
        dy = 1, dx = -1, len = min(a.H - y0, x0 + 1);
    }
    sgm_march<DPL>(a, pix0, y0, x0, dy, dx, len, a.init != 0);
    sgm_march<DPL>(a, pix0, y0 + (len - 1) * dy, x0 + (len - 1) * dx, -dy, -dx, len, false);
}

struct SgmSelectArgs {
    const uint16_t *S;
    int16_t *iR;                  // [n][H][W]: right-view winner, -1 where no candidate lies in the image
    float *out;
    float *right_out;             // [n][H][W] f32(dmin + iR), invalid where iR = -1; NULL: not written
    int n, H, W, dmin, D, Dp;
    int uniqueness, lr, subpixel;
    float lr_max_diff, invalid;
};

// key of a candidate: the smaller S wins, then the smaller i (S <= 2040 < 2^11, i < 2^8)
__device__ __forceinline__ unsigned sgm_key(unsigned s, int i) { return (s << 8) | (unsigned)i; }

// iR(y, x') = the smallest i minimising S(y, x' + dmin + i, i) over x' + dmin + i <= W - 1.  One wave per pixel.
// With right_out, the right-view map is written beside it.
template <int DPL>
__global__ __launch_bounds__(SGM_THREADS) void k_sgm_right_wta(SgmSelectArgs a) {
    const int lane = threadIdx.x & 63;
    const size_t pixels = (size_t)a.n * a.H * a.W;
    const size_t waves = (size_t)gridDim.x * (SGM_THREADS / 64);
    for (size_t p = (size_t)blockIdx.x * (SGM_THREADS / 64) + (threadIdx.x >> 6); p < pixels; p += waves) {
        const int x = (int)(p % a.W);
        unsigned key = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < DPL; ++k) {
            const int i = lane * DPL + k;
            const int xl = x + a.dmin + i;
            if (i < a.D && xl <= a.W - 1) key = min(key, sgm_key(a.S[(p + (xl - x)) * a.Dp + i], i));
        }
        key = __ockl_wfred_min_u32(key);
        if (lane == 0) {
            const bool none = key == 0xFFFFFFFFu;
            a.iR[p] = none ? (int16_t)-1 : (int16_t)(key & 0xFFu);
            if (a.right_out) a.right_out[p] = none ? a.invalid : (float)(a.dmin + (int)(key & 0xFFu));
        }
    }
}

template <int DPL>
__global__ __launch_bounds__(SGM_THREADS) void k_sgm_select(SgmSelectArgs a) {
    const int lane = threadIdx.x & 63;
    const int i0 = lane * DPL;
    using V = typename SgmVec<DPL>::T;
    const int vpp = a.Dp / DPL;
    const size_t pixels = (size_t)a.n * a.H * a.W;
    const size_t waves = (size_t)gridDim.x * (SGM_THREADS / 64);
    for (size_t p = (size_t)blockIdx.x * (SGM_THREADS / 64) + (threadIdx.x >> 6); p < pixels; p += waves) {
        const int x = (int)(p % a.W);
        unsigned s[DPL];
        if (i0 < a.Dp) sgm_unpack<DPL>(((const V *)(a.S + p * a.Dp))[lane], s);
        unsigned key = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < DPL; ++k)
            if (i0 + k < a.D) key = min(key, sgm_key(s[k], i0 + k));
        key = __ockl_wfred_min_u32(key);
        const int ist = (int)(key & 0xFFu);
        const unsigned s0 = key >> 8;
        const int d = a.dmin + ist;
        bool bad = x - d < 0;                                                      // (a)
        if (a.uniqueness) {                                                        // (b)
            unsigned far = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < DPL; ++k) {
                const int i = i0 + k;
                if (i < a.D && abs(i - ist) > 1) far = min(far, s[k]);
            }
            far = __ockl_wfred_min_u32(far);
            if (far != 0xFFFFFFFFu && far * (unsigned)(100 - a.uniqueness) < s0 * 100u) bad = true;
        }
        if (lane == 0) {
            if (!bad && a.lr) {                                                    // (c): x - d >= 0 here
                const int ir = a.iR[p - d];
                if ((float)abs(a.dmin + ir - d) > a.lr_max_diff) bad = true;
            }
            float v = (float)d;
            if (a.subpixel && ist > 0 && ist < a.D - 1) {
                const int sm = a.S[p * a.Dp + ist - 1], sp = a.S[p * a.Dp + ist + 1];
                const int den = sm + sp - 2 * (int)s0;
                if (den > 0) v = __fadd_rn(v, __fdiv_rn((float)(sm - sp), (float)(2 * den)));
            }
            a.out[p] = bad ? a.invalid : v;
        }
    }
}

}  // namespace smx
