// k_synthesis.h -- right-view synthesis head (include/stereo_mi355x.h: smx_synthesize_right_view): the bilinear
// upsampling of the low-resolution probability volume, the D shifted copies of the left frame, their product, the sum
// over the disparity axis and the rescale to 0..255 in one launch.  Neither the upsampled volume nor the shifted stack
// exists anywhere: both are consumed where they are produced.
//
// A workgroup of SYN_THREADS threads owns a SYN_TW x SYN_TH output tile of one frame; a lane owns one column and
// marches SYN_ROWS consecutive rows of it.  The disparity axis is walked in chunks of a.dc planes (the host's choice,
// synthesis_chunk below: what fits SYN_LDS_FLOATS).  Per chunk the workgroup stages
//   - the tile's left rows, SYN_TW + dc - 1 columns per channel and row (pixel (X, Y) reads columns Y + d of its own
//     row), as float32: a u8 frame is divided by 255 here, once per staged value.  Layout [column][channel, row] with an
//     odd stride: a lane's values of one d sit at compile-time offsets from one address, and lanes fall on distinct banks;
//   - the low-resolution patch under the tile, [patch element][plane] with an odd stride, for the same two reasons;
// and every lane then adds the chunk's terms to accumulators that stay in registers, so the order in d is 0, 1, ...,
// D-1 whatever the chunk length.  The rule does the horizontal lerp first, so `top` and `bot` of a column belong to a
// pair of low-resolution rows: where the wave's rows 0, 1 and its rows 2, 3 each fall between one pair (always for S a
// multiple of 4), they are computed once per two rows, otherwise per row.  The choice is uniform over the wave (a lane is
// a column) and changes no bit.  Every operation is one float32 round-to-nearest (explicit __f*_rn, -ffp-contract=off),
// so the result depends neither on the tile nor on the chunk.
#pragma once
#include "smx_common.h"

namespace smx {

constexpr int SYN_TW = 64;                        // tile columns: one per lane
constexpr int SYN_ROWS = 4;                       // consecutive output rows of one lane
constexpr int SYN_THREADS = 256;
constexpr int SYN_WAVES = SYN_THREADS / SYN_TW;
constexpr int SYN_TH = SYN_WAVES * SYN_ROWS;      // tile rows
constexpr int SYN_LDS_FLOATS = 14 * 1024;         // 56 KB; D = 65, S = 4, C = 3 take 53.2 KB in one chunk: three workgroups per CU
static_assert(SYN_LDS_FLOATS * sizeof(float) <= 64 * 1024, "k_synthesis: at most 64 KB of LDS per workgroup");

struct SynArgs {
    const float *prob;                            // [n][D][h][w]
    const void *left;                             // [n][C][H][W] f32 or u8
    float *out;                                   // [n][C][H][W]
    int n, D, h, w, S, H, W, tiles_x;
    int dc;                                       // planes per chunk
};

// Source indices and weights of output index t (the half-pixel rule, in integers).
struct SynTap {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ int syn_i0(int t, int S) { return max(2 * t + 1 - S, 0) / (2 * S); }
__device__ __forceinline__ SynTap syn_tap(int t, int S, int len) {
    const int u = max(2 * t + 1 - S, 0);
    SynTap p;
    p.i0 = u / (2 * S);
    p.i1 = min(p.i0 + 1, len - 1);
    p.l1 = __fdiv_rn((float)(u % (2 * S)), (float)(2 * S));
    p.l0 = __fsub_rn(1.0f, p.l1);
    return p;
}

// Low-resolution rows (columns) under `tile` consecutive output rows (columns), at most: the first source indices of
// the tile's ends differ by at most (tile - 1) / S + 1, the second index adds one, and the count one more.
__host__ __device__ constexpr int syn_patch_extent(int tile, int S, int len) {
    return (tile - 1) / S + 3 < len ? (tile - 1) / S + 3 : len;
}
__host__ __device__ constexpr int syn_left_stride(int C) { return C * SYN_TH + 1; }      // odd
__host__ __device__ constexpr int syn_patch_stride(int D_chunk) { return D_chunk | 1; }  // odd

__host__ __device__ constexpr int syn_lds_floats(int C, int D_chunk, int S, int h, int w) {
    return (SYN_TW + D_chunk - 1) * syn_left_stride(C) +
           syn_patch_extent(SYN_TH, S, h) * syn_patch_extent(SYN_TW, S, w) * syn_patch_stride(D_chunk);
}

// The longest chunk that fits SYN_LDS_FLOATS (one plane always does: S = 1 has 18 x 66 patch elements).
inline int synthesis_chunk(int C, int D, int S, int h, int w) {
    const int elements = syn_patch_extent(SYN_TH, S, h) * syn_patch_extent(SYN_TW, S, w);
    const int dc = (SYN_LDS_FLOATS - (SYN_TW - 1) * syn_left_stride(C) - elements) / (syn_left_stride(C) + elements);
    return dc < 1 ? 1 : (dc > D ? D : dc);
}

// The chunk's terms of one lane: d = 0 .. nd-1 in order.  SHARE: rows per (top, bot).  lcol: the lane's staged column at
// the wave's first row; p0 / p1: the patch at the lane's two source columns; o0 / o1: the rows' patch-element offsets.
template <int C, int SHARE>
__device__ __forceinline__ void syn_march(float (&acc)[SYN_ROWS][C], int nd, const float *lcol, const float *p0,
                                          const float *p1, int PS, const int (&o0)[SYN_ROWS], const int (&o1)[SYN_ROWS],
                                          const float (&a0)[SYN_ROWS], const float (&a1)[SYN_ROWS], float b0, float b1) {
    constexpr int NS = SYN_ROWS / SHARE, LS = syn_left_stride(C);
    const float *p00[NS], *p01[NS], *p10[NS], *p11[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        p00[s] = p0 + o0[s * SHARE] * PS, p01[s] = p1 + o0[s * SHARE] * PS;
        p10[s] = p0 + o1[s * SHARE] * PS, p11[s] = p1 + o1[s * SHARE] * PS;
    }
#pragma unroll 2
    for (int d = 0; d < nd; ++d) {
        float top[NS], bot[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            top[s] = __fadd_rn(__fmul_rn(b0, p00[s][d]), __fmul_rn(b1, p01[s][d]));
            bot[s] = __fadd_rn(__fmul_rn(b0, p10[s][d]), __fmul_rn(b1, p11[s][d]));
        }
#pragma unroll
        for (int j = 0; j < SYN_ROWS; ++j) {
            const float q = __fadd_rn(__fmul_rn(a0[j], top[j / SHARE]), __fmul_rn(a1[j], bot[j / SHARE]));
#pragma unroll
            for (int c = 0; c < C; ++c)
                acc[j][c] = __fadd_rn(acc[j][c], __fmul_rn(q, lcol[d * LS + c * SYN_TH + j]));
        }
    }
}

// RESCALE: the rule's last step (smx_synthesize_right_view); without it the sums themselves are stored, the training
// form of smx_synthesis_head_forward.
template <int C, bool F32, bool RESCALE = true>
__global__ __launch_bounds__(SYN_THREADS) void k_synthesis(SynArgs a) {
    extern __shared__ float lds[];
    constexpr int LS = syn_left_stride(C);
    const int PS = syn_patch_stride(a.dc);
    float *lv = lds;                              // [SYN_TW + dc - 1 columns][LS]: row k = channel * SYN_TH + tile row
    float *pp = lds + (SYN_TW + a.dc - 1) * LS;   // [patch element][PS]
    const int S = a.S;
    const int x0 = (blockIdx.x / a.tiles_x) * SYN_TH, y0 = (blockIdx.x % a.tiles_x) * SYN_TW;       // row, column
    const int lane = threadIdx.x % SYN_TW;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / SYN_TW);
    const int Y = y0 + lane;
    const size_t HW = (size_t)a.H * a.W, hw = (size_t)a.h * a.w;
    // the patch under the tile: rows pr_lo .. pr_lo + pr_n - 1, columns pc_lo .. pc_lo + pc_n - 1
    const int pr_lo = syn_i0(x0, S), pc_lo = syn_i0(y0, S);
    const int pr_n = min(syn_i0(min(x0 + SYN_TH, a.H) - 1, S) + 1, a.h - 1) - pr_lo + 1;
    const int pc_n = min(syn_i0(min(y0 + SYN_TW, a.W) - 1, S) + 1, a.w - 1) - pc_lo + 1;
    const int RC = pr_n * pc_n;
    // this lane's column (lanes right of the image take the last column's taps and store nothing)
    const SynTap col = syn_tap(min(Y, a.W - 1), S, a.w);
    const float *p0 = pp + (col.i0 - pc_lo) * PS, *p1 = pp + (col.i1 - pc_lo) * PS;
    // this wave's rows (rows below the image take the last row's taps and store nothing)
    int o0[SYN_ROWS], o1[SYN_ROWS];
    float a0[SYN_ROWS], a1[SYN_ROWS];
#pragma unroll
    for (int j = 0; j < SYN_ROWS; ++j) {
        const SynTap row = syn_tap(min(x0 + wv * SYN_ROWS + j, a.H - 1), S, a.h);
        o0[j] = (row.i0 - pr_lo) * pc_n, o1[j] = (row.i1 - pr_lo) * pc_n;
        a0[j] = row.l0, a1[j] = row.l1;
    }
    const bool pairs = o0[0] == o0[1] && o1[0] == o1[1] && o0[2] == o0[3] && o1[2] == o1[3];
    // patch staging: thread -> patch element e and, where the patch is smaller than the workgroup, one of `groups`
    // interleaved sets of planes
    const int groups = RC < SYN_THREADS ? SYN_THREADS / RC : 1;
    const int grp = threadIdx.x / RC;

    for (int m = blockIdx.y; m < a.n; m += gridDim.y) {
        float acc[SYN_ROWS][C];
#pragma unroll
        for (int j = 0; j < SYN_ROWS; ++j)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[j][c] = 0.0f;
        for (int d0 = 0; d0 < a.D && y0 + d0 < a.W; d0 += a.dc) {       // past W - y0 no lane of the tile has a term
            const int nd = min(a.dc, a.D - d0);
            __syncthreads();                      // the previous chunk is read
            const int cols = min(SYN_TW + nd - 1, a.W - y0 - d0);       // columns right of the image are never read
            for (int k = wv; k < C * SYN_TH; k += SYN_WAVES) {
                const int X = x0 + k % SYN_TH;
                if (X >= a.H) continue;
                const size_t src = ((size_t)m * C + k / SYN_TH) * HW + (size_t)X * a.W + y0 + d0;
#pragma unroll 2
                for (int c = lane; c < cols; c += SYN_TW) {
                    if constexpr (F32) lv[c * LS + k] = ((const float *)a.left)[src + c];
                    else lv[c * LS + k] = __fdiv_rn((float)((const uint8_t *)a.left)[src + c], 255.0f);
                }
            }
            if (grp < groups) {
                const float *pm = a.prob + ((size_t)m * a.D + d0) * hw;
                for (int e = threadIdx.x - grp * RC; e < RC; e += SYN_THREADS) {
                    const int r = e / pc_n;
                    const float *src = pm + (size_t)(pr_lo + r) * a.w + pc_lo + (e - r * pc_n);
#pragma unroll 4
                    for (int d = grp; d < nd; d += groups) pp[e * PS + d] = src[(size_t)d * hw];
                }
            }
            __syncthreads();
            const int ndl = min(nd, a.W - Y - d0);                     // this lane's terms: Y + d < W
            const float *lcol = lv + lane * LS + wv * SYN_ROWS;
            if (pairs) syn_march<C, 2>(acc, ndl, lcol, p0, p1, PS, o0, o1, a0, a1, col.l0, col.l1);
            else syn_march<C, 1>(acc, ndl, lcol, p0, p1, PS, o0, o1, a0, a1, col.l0, col.l1);
        }
        if (Y >= a.W) continue;                   // on to the next frame's barriers
#pragma unroll
        for (int j = 0; j < SYN_ROWS; ++j) {
            const int X = x0 + wv * SYN_ROWS + j;
            if (X >= a.H) break;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float *dst = a.out + ((size_t)m * C + c) * HW + (size_t)X * a.W + Y;
                if constexpr (RESCALE) *dst = fminf(fmaxf(__fadd_rn(__fmul_rn(acc[j][c], 255.0f), 0.5f), 0.0f), 255.0f);
                else *dst = acc[j][c];
            }
        }
    }
}

}  // namespace smx
