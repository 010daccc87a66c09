// k_synthesis_grad.h -- backward of the right-view synthesis head (include/stereo_mi355x.h: smx_synthesis_head_backward):
// the gradient of the low-resolution probability volume from the gradient of the view, in one launch.  Neither the
// per-plane product G (full resolution) nor its horizontal transpose T exists in global memory: G lives in registers for
// one term, T in LDS for U planes at a time.
//
// A workgroup owns ti x tj low-resolution cells of one frame and the rows x columns of the view that reach them: with
// first(k) = k <= 0 ? 0 : S k + S / 2 (the first output index whose first tap is k), cell k is reached by the output
// indices first(k - 1) .. min(first(k + 1), len) - 1, which are contiguous: first those whose SECOND tap is k, then those
// whose first tap is k (and, for the last cell, whose second tap is k as well).  That is 2S indices in the interior and at
// most 2S + S / 2 at the borders (NT).
//   - Horizontal transpose: a lane owns one view row X and one low-resolution column j.  It keeps its strip of g (C x NT
//     values) and the strip's weights in registers for the whole frame, and per step of U planes reads a window of
//     NT + U - 1 staged left values per channel: plane d + u uses the window's elements u .. u + NT - 1.  It walks the
//     strip in ascending Y, so T[X][j] has the rule's order, and recomputes the G values it shares with its neighbours.
//   - Vertical transpose: T of U planes goes through LDS (two buffers, so one barrier per step); a lane then owns one cell
//     (i, j) of one plane and walks the rows first(i - 1) .. in ascending X.  Where one round of the workgroup covers the
//     step's cells, a lane's cell is the same in every step and its rows are a strip with the weights in registers, like
//     the horizontal one; otherwise (S < 4) the row taps come from a table in LDS.
// The left rows are staged per chunk of dc planes as in k_synthesis.h ([channel][row][column], an odd row stride; a u8
// frame is divided by 255 here).  Every operation is one float32 round-to-nearest (explicit __f*_rn, -ffp-contract=off),
// every predicate of the rule is a real branch (a skipped term is not added as zero), so the result depends neither on
// the tile nor on the chunk nor on U.
#pragma once
#include "k_synthesis.h"

namespace smx {

constexpr int SYG_LDS_FLOATS = 14 * 1024;         // 56 KB; D = 65, S = 4, C = 3 take 50.7 KB in one chunk
static_assert(SYG_LDS_FLOATS * sizeof(float) <= 64 * 1024, "k_synthesis_grad: at most 64 KB of LDS per workgroup");
constexpr int SYG_MAX_THREADS = 256;

// The tile and the instantiation of a scale: rows (a power of two) x tj lanes; NT >= 2S + S / 2 strip terms; U planes a step.
struct SynGradShape {
    int rows_log2, tj_log2, NT, U;
};
inline SynGradShape syn_grad_shape(int S) {
    if (S <= 4) return {5, 3, 10, 4};
    if (S <= 8) return {5, 3, 20, 2};
    return {6, 1, 40, 1};
}

struct SynGradArgs {
    const float *g;                               // [n][C][H][W]
    const void *left;                             // [n][C][H][W] f32 or u8
    float *out;                                   // [n][D][h][w]
    int n, D, h, w, S, H, W;
    int rows_log2, tj_log2;                       // lanes along X, lanes along j
    int ti;                                       // low-resolution rows of a tile: rows / S - 1 (>= 2)
    int tiles_j;
    int dc;                                       // planes per staged chunk: a multiple of U
    int rs;                                       // floats of a staged row (odd)
};

__host__ __device__ constexpr int syg_first(int k, int S) { return k <= 0 ? 0 : S * k + S / 2; }
// One plane of T: [row][tj + 1], plus one float so that the planes of a step start on different banks.
__host__ __device__ constexpr int syg_t_plane(int rows, int tj) { return rows * (tj + 1) + 1; }
// A staged row holds every column a lane's window can touch: the last lane's strip starts S (tj - 1) + S / 2 columns
// (at most) right of the tile's first, and reads NT + dc - 1 from there.
__host__ __device__ constexpr int syg_row_floats(int S, int tj, int NT, int dc) {
    return (S * (tj - 1) + S / 2 + NT + dc - 1) | 1;
}
__host__ __device__ constexpr int syg_lds_floats(int C, int S, int rows, int tj, int NT, int U, int dc) {
    return C * rows * syg_row_floats(S, tj, NT, dc) + 2 * U * syg_t_plane(rows, tj) + 3 * rows;
}

// The longest chunk (a multiple of U) that fits SYG_LDS_FLOATS; one step always does.
inline int synthesis_grad_chunk(int C, int D, int S) {
    const SynGradShape sh = syn_grad_shape(S);
    const int rows = 1 << sh.rows_log2, tj = 1 << sh.tj_log2;
    const int fixed = 2 * sh.U * syg_t_plane(rows, tj) + 3 * rows;
    int dc = (SYG_LDS_FLOATS - fixed) / (C * rows) - (S * (tj - 1) + S / 2 + sh.NT);      // `| 1` adds at most one float
    dc -= dc % sh.U;
    const int all = (D + sh.U - 1) / sh.U * sh.U;
    return dc < sh.U ? sh.U : (dc > all ? all : dc);
}

// T of U consecutive planes for one lane.  v: the lane's staged row at its strip's first column and the step's first
// plane, channel stride cs.  FULL (uniform over the workgroup): every lane has the interior's 2S terms and every term's
// column is inside the frame.  Otherwise nk terms, of which those with Y + d < W count (room = W - Ylo - d); from kB on
// `both` taps are this cell (the last column of the volume).
template <int C, int NT, int U, bool FULL>
__device__ __forceinline__ void syg_strip(float (&T)[U], const float (&g)[C][NT], const float (&wk)[NT], const float *v,
                                          int cs, int S, int w, int Ylo, int nk, int kB, bool both, int room) {
    float win[C][NT + U - 1];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int t = 0; t < NT + U - 1; ++t) win[c][t] = v[c * cs + t];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        float acc = 0.0f;
        const int lim = FULL ? 2 * S : min(nk, room - u);
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            if (k < lim) {
                float G = __fmul_rn(g[0][k], win[0][k + u]);
#pragma unroll
                for (int c = 1; c < C; ++c) G = __fadd_rn(G, __fmul_rn(g[c][k], win[c][k + u]));
                acc = __fadd_rn(acc, __fmul_rn(wk[k], G));
                if (!FULL && both && k >= kB) acc = __fadd_rn(acc, __fmul_rn(syn_tap(Ylo + k, S, w).l1, G));
            }
        }
        T[u] = acc;
    }
}

// SC: the scale where it is known at compile time (the strips' loops then have no tests in the interior), else 0.
template <int C, bool F32, int NT, int U, int SC>
__global__ __launch_bounds__(SYG_MAX_THREADS) void k_synthesis_grad(SynGradArgs a) {
    extern __shared__ float lds[];
    static_assert(SC >= 0 && SC <= 8, "k_synthesis_grad: a compile-time scale has the 32 x 8 tile of syn_grad_shape");
    const int S = SC ? SC : a.S, RL = SC ? 5 : a.rows_log2, TL = SC ? 3 : a.tj_log2, ROWS = 1 << RL, TJ = 1 << TL;
    const int TI = SC ? 32 / (SC ? SC : 1) - 1 : a.ti;
    const int threads = ROWS * TJ;                // == blockDim.x
    const int RS = a.rs, CS = ROWS * RS, TP = syg_t_plane(ROWS, TJ);
    float *lv = lds;                              // [C][ROWS][RS]
    float *tb = lv + C * CS;                      // [2][U][TP]
    float *ra0 = tb + 2 * U * TP, *ra1 = ra0 + ROWS;     // row taps of the tile's rows
    int *rr0 = (int *)(ra1 + ROWS);
    const int tid = threadIdx.x;
    const int i_lo = (blockIdx.x / a.tiles_j) * TI, j_lo = (blockIdx.x % a.tiles_j) * TJ;
    const int i_n = min(TI, a.h - i_lo), j_n = min(TJ, a.w - j_lo);
    const int Xbase = syg_first(i_lo - 1, S), Xend = min(syg_first(i_lo + i_n, S), a.H);   // Xend - Xbase <= ROWS
    const int Ybase = syg_first(j_lo - 1, S), Yend = min(syg_first(j_lo + j_n, S), a.W);
    const size_t HW = (size_t)a.H * a.W, hw = (size_t)a.h * a.w;
    // horizontal lane: row X, column j
    const int x = tid & (ROWS - 1), jj = tid >> RL;
    const int X = Xbase + x, j = j_lo + jj;
    const bool active = X < Xend && jj < j_n;
    const int Ylo = syg_first(j - 1, S);
    const int nk = active ? min(syg_first(j + 1, S), a.W) - Ylo : 0;       // <= NT
    const int kB = syg_first(j, S) - Ylo;         // terms below kB: second tap; from kB on: first tap
    const bool both = j == a.w - 1;
    float wk[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const SynTap t = syn_tap(min(Ylo + k, a.W - 1), S, a.w);
        wk[k] = k < kB ? t.l1 : t.l0;
    }
    const bool tile_full = j_lo >= 2 && j_lo + TJ <= a.w - 1;              // then nk = 2S, kB = S and !both everywhere
    // vertical lane: column vj and, per round, one (plane, row) pair q = u * TI + ii
    const int vj = tid & (TJ - 1), vq = tid >> TL;
    const int vu0 = vq / TI, vi0 = vq - vu0 * TI;
    // Where one round covers the step's cells (uniform), the lane's cell is the same in every step and its rows are a
    // strip like the horizontal one: nv terms from row xv_lo of the tile, the second tap below kBv, weights in registers.
    const bool one_round = U * TI <= ROWS;
    const int vi = i_lo + vi0;
    const bool vcell = one_round && vu0 < U && vi0 < i_n && vj < j_n;
    const int xv_lo = syg_first(vi - 1, S) - Xbase;
    const int nv = vcell ? min(syg_first(vi + 1, S), a.H) - syg_first(vi - 1, S) : 0;      // <= NT
    const int kBv = syg_first(vi, S) - syg_first(vi - 1, S);
    const bool vboth = vi == a.h - 1;
    float wr[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        const SynTap t = syn_tap(min(Xbase + xv_lo + k, a.H - 1), S, a.h);
        wr[k] = k < kBv ? t.l1 : t.l0;
    }
    if (tid < ROWS) {
        const SynTap t = syn_tap(min(Xbase + tid, a.H - 1), S, a.h);
        ra0[tid] = t.l0, ra1[tid] = t.l1, rr0[tid] = t.i0;
    }
    const int waves = threads / 64, wv = __builtin_amdgcn_readfirstlane(tid / 64), lane = tid % 64;

    for (int m = blockIdx.y; m < a.n; m += gridDim.y) {
        float g[C][NT];
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int k = 0; k < NT; ++k)
                g[c][k] = k < nk ? a.g[((size_t)m * C + c) * HW + (size_t)X * a.W + Ylo + k] : 0.0f;
        int step = 0;
        for (int d0 = 0; d0 < a.D; d0 += a.dc) {
            const int nd = min(a.dc, a.D - d0);
            __syncthreads();                      // the previous chunk is read (and the row taps are written)
            const int cols = min(Yend - Ybase + nd - 1, a.W - Ybase - d0);  // columns right of the frame are never read
            for (int k = wv; k < C * (Xend - Xbase); k += waves) {
                const int ch = k / (Xend - Xbase), xr = k - ch * (Xend - Xbase);
                const size_t src = ((size_t)m * C + ch) * HW + (size_t)(Xbase + xr) * a.W + Ybase + d0;
                float *dst = lv + ch * CS + xr * RS;
#pragma unroll 2
                for (int c = lane; c < cols; c += 64) {
                    if constexpr (F32) dst[c] = ((const float *)a.left)[src + c];
                    else dst[c] = __fdiv_rn((float)((const uint8_t *)a.left)[src + c], 255.0f);
                }
            }
            __syncthreads();
            for (int ds = 0; ds < nd; ds += U, ++step) {
                const int d = d0 + ds;
                float *tw = tb + (step & 1) * U * TP;
                if (active) {
                    float T[U];
                    const float *v = lv + x * RS + (Ylo - Ybase) + ds;
                    if (tile_full && Yend + d + U - 1 <= a.W)
                        syg_strip<C, NT, U, true>(T, g, wk, v, CS, S, a.w, Ylo, nk, kB, both, 0);
                    else
                        syg_strip<C, NT, U, false>(T, g, wk, v, CS, S, a.w, Ylo, nk, kB, both, a.W - Ylo - d);
#pragma unroll
                    for (int u = 0; u < U; ++u) tw[u * TP + x * (TJ + 1) + jj] = T[u];
                }
                __syncthreads();                  // the other buffer is free again after the next step's barrier
                if (one_round) {
                    if (d + vu0 < a.D && nv > 0) {
                        const float *tr = tw + vu0 * TP + xv_lo * (TJ + 1) + vj;
                        float acc = 0.0f;
#pragma unroll
                        for (int k = 0; k < NT; ++k) {
                            if (k < nv) {
                                const float t = tr[k * (TJ + 1)];
                                acc = __fadd_rn(acc, __fmul_rn(wr[k], t));
                                if (vboth && k >= kBv) acc = __fadd_rn(acc, __fmul_rn(ra1[xv_lo + k], t));
                            }
                        }
                        a.out[((size_t)m * a.D + d + vu0) * hw + (size_t)vi * a.w + j_lo + vj] = acc;
                    }
                    continue;
                }
                for (int q = vq; q < U * TI; q += ROWS) {
                    int u, ii;
                    if (q == vq) u = vu0, ii = vi0;
                    else u = q / TI, ii = q - u * TI;
                    const int i = i_lo + ii;
                    if (d + u >= a.D || ii >= i_n || vj >= j_n) continue;
                    const int x_lo = syg_first(i - 1, S) - Xbase, x_hi = min(syg_first(i + 1, S), a.H) - Xbase;
                    const float *tr = tw + u * TP + vj;
                    float acc = 0.0f;
                    for (int xr = x_lo; xr < x_hi; ++xr) {
                        const float t = tr[xr * (TJ + 1)];
                        const int r0 = rr0[xr];
                        if (r0 == i) acc = __fadd_rn(acc, __fmul_rn(ra0[xr], t));
                        if (min(r0 + 1, a.h - 1) == i) acc = __fadd_rn(acc, __fmul_rn(ra1[xr], t));
                    }
                    a.out[((size_t)m * a.D + d + u) * hw + (size_t)i * a.w + j_lo + vj] = acc;
                }
            }
        }
    }
}

}  // namespace smx
