// k_wls.h -- image-guided weighted least squares filter (include/stereo_mi355x.h: smx_wls_filter).
//
// One iteration t of the rule is two launches on the caller's stream, so a call of T iterations is 2T launches:
//   1. k_wls_rows: every row of U and V solved with the Thomas algorithm, one lane per row.  A workgroup owns 64 rows;
//      wave 0 solves them, one lane per row, from 64 x WLS_TW tiles in LDS, and waves 1..3 move the tiles: while the
//      solver works on chunk c they store chunk c-1's results and load chunk c+1 into the other buffer, so the solver
//      never waits on global memory.  The movers also compute each pixel's coupling R_j = lambda * w(g_j, g_{j+1}) (it
//      depends on the guide only), so the solver reads three independent values per step and its recurrence waits on
//      nothing but itself.  The forward sweep writes e, y_U and y_V over R, U and V in the tile; the movers store them to the E, U and V planes, and the back sweep reads them in reverse the same
//      way.  The last two forward chunks never leave LDS: the back sweep starts on them.  With t == 0 the forward
//      sweep builds U and V from `in` and `confidence` as it goes.
//   2. k_wls_cols: every column solved, one lane per column, so each step's loads and stores are coalesced across the
//      lanes; loads run WLS_PF steps ahead of the recurrence.  With t == T-1 the back sweep writes out = U / V.
// Every operation is one float32 round-to-nearest (explicit __f*_rn, -ffp-contract=off) and 1/den is the correctly
// rounded division, in the order the rule states, so the result does not depend on the split of the work.  r and e
// depend only on the guide and lambda: U and V of a line share them.
#pragma once
#include "smx_common.h"

namespace smx {

constexpr int WLS_LINES = 64;                    // rows per workgroup of k_wls_rows: one per lane of the solving wave
constexpr int WLS_TW = 32;                       // columns per staged chunk
constexpr int WLS_TP = WLS_TW + 1;               // tile pitch: conflict-free lane-per-row reads
constexpr int WLS_MOVERS = 3;                    // waves that move tiles
constexpr int WLS_ROW_THREADS = 64 * (1 + WLS_MOVERS);
constexpr int WLS_MOVE = 64 * WLS_MOVERS;
constexpr int WLS_PER_MOVER = (WLS_LINES * WLS_TW + WLS_MOVE - 1) / WLS_MOVE;    // chunk elements per mover thread
constexpr int WLS_COL_THREADS = 64;
constexpr int WLS_PF = 8;                        // k_wls_cols: steps of loads in flight ahead of the forward recurrence
constexpr int WLS_PB = 16;                       // ... ahead of the back sweep (a short chain: deeper)

// The range table travels in the kernel arguments (1 KB): the call copies nothing to the device.
struct WlsTable {
    float range[256];
};

struct WlsArgs {
    const float *in, *conf, *guide;
    float *U, *V, *E;                            // workspace planes, [n][H][W] each
    float *out;
    int n, H, W;
    float lambda, min_weight, invalid;
    int first;                                   // k_wls_rows: build U and V from in / conf (t == 0)
    int last;                                    // k_wls_cols: write out (t == T-1)
};

__device__ __forceinline__ int wls_range_index(float gp, float gq) {
    const float a = fabsf(__fsub_rn(gp, gq));
    return a < 255.0f ? (int)a : 255;            // NaN and >= 255: 255
}

// The rule's 1. and 2.: U and V of one pixel.
__device__ __forceinline__ void wls_planes(float d, bool has_conf, float k, float invalid, float &u, float &v) {
    const bool valid = __builtin_isfinite(d) && d != invalid;
    const float c = !valid ? 0.0f : !has_conf ? 1.0f : k > 0.0f ? fminf(k, 1.0f) : 0.0f;
    u = valid ? __fmul_rn(d, c) : 0.0f;
    v = c;
}

// One forward step j of the Thomas algorithm; e, yu, yv hold step j-1's values on entry (unused when j == 0).
__device__ __forceinline__ void wls_forward(bool j0, float L, float R, float fu, float fv, float &e, float &yu,
                                            float &yv) {
    const float b = __fadd_rn(__fadd_rn(1.0f, L), R);
    if (j0) {
        const float r = __fdiv_rn(1.0f, b);
        e = __fmul_rn(R, r);
        yu = __fmul_rn(fu, r);
        yv = __fmul_rn(fv, r);
    } else {
        const float r = __fdiv_rn(1.0f, __fsub_rn(b, __fmul_rn(L, e)));
        e = __fmul_rn(R, r);
        yu = __fmul_rn(__fadd_rn(fu, __fmul_rn(L, yu)), r);
        yv = __fmul_rn(__fadd_rn(fv, __fmul_rn(L, yv)), r);
    }
}

// The rule's 6.
__device__ __forceinline__ float wls_output(float u, float v, float min_weight, float invalid) {
    if (!(v > min_weight)) return invalid;
    const float q = __fdiv_rn(u, v);
    return q == q ? q : __uint_as_float(0x7FC00000u);
}

__global__ __launch_bounds__(WLS_ROW_THREADS) void k_wls_rows(WlsArgs a, WlsTable tab) {
    __shared__ float rw[256];
    __shared__ float tile[2][3][WLS_LINES][WLS_TP];      // [buffer][plane][row][column]
    for (int k = threadIdx.x; k < 256; k += WLS_ROW_THREADS) rw[k] = tab.range[k];
    const int lane = threadIdx.x & 63;
    const bool solver = threadIdx.x < 64;
    const int mt = threadIdx.x - 64;                     // mover thread 0 .. 64 * WLS_MOVERS - 1
    const int W = a.W;
    const size_t lines = (size_t)a.n * a.H;
    const int chunks = (W + WLS_TW - 1) / WLS_TW;
    const bool has_conf = a.conf != nullptr;
    const float lam = a.lambda;
    __syncthreads();
    for (size_t line0 = (size_t)blockIdx.x * WLS_LINES; line0 < lines; line0 += (size_t)gridDim.x * WLS_LINES) {
        const int nl = (int)min((size_t)WLS_LINES, lines - line0);
        const size_t base = line0 * W;                   // pixel (row line0 + rr, column x) at base + rr * W + x

        // Movers.  Element i of mover thread mt is k = mt + i * WLS_MOVE, (rr, cc) = (k / WLS_TW, k % WLS_TW), in every
        // operation below, so an element of a buffer is only ever touched by one mover thread, in program order (store
        // before the next load).  Each operation issues all its global loads before it uses one: addresses of elements
        // outside the map are clamped to pixel `base`, loaded and not used.
        auto elem = [&](int c, int i, size_t &p, int &rr, int &cc) {
            const int k = mt + i * WLS_MOVE;
            rr = k / WLS_TW, cc = k % WLS_TW;
            const bool ok = k < WLS_LINES * WLS_TW && rr < nl && c * WLS_TW + cc < W;
            p = ok ? base + (size_t)rr * W + c * WLS_TW + cc : base;
            return ok;
        };
        auto load_fwd = [&](int c, int buf) {
            float g0[WLS_PER_MOVER], g1[WLS_PER_MOVER], u[WLS_PER_MOVER], v[WLS_PER_MOVER];
#pragma unroll
            for (int i = 0; i < WLS_PER_MOVER; ++i) {
                size_t p;
                int rr, cc;
                const bool ok = elem(c, i, p, rr, cc);
                const bool right = ok && c * WLS_TW + cc < W - 1;
                g0[i] = a.guide[p];
                g1[i] = a.guide[right ? p + 1 : p];
                u[i] = a.first ? a.in[p] : a.U[p];
                v[i] = !a.first ? a.V[p] : has_conf ? a.conf[p] : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < WLS_PER_MOVER; ++i) {
                size_t p;
                int rr, cc;
                if (!elem(c, i, p, rr, cc)) continue;
                // R_j = s_j, off the solver's path: it depends on the guide and lambda only
                tile[buf][0][rr][cc] =
                    c * WLS_TW + cc < W - 1 ? __fmul_rn(lam, rw[wls_range_index(g0[i], g1[i])]) : 0.0f;
                tile[buf][1][rr][cc] = u[i];
                tile[buf][2][rr][cc] = v[i];
            }
        };
        // planes: 3 (e -> E, y_U -> U, y_V -> V) after the forward sweep, 2 (x_U -> U, x_V -> V) after the back sweep
        auto store = [&](int c, int buf, bool with_e) {
#pragma unroll
            for (int i = 0; i < WLS_PER_MOVER; ++i) {
                size_t p;
                int rr, cc;
                if (!elem(c, i, p, rr, cc)) continue;
                if (with_e) a.E[p] = tile[buf][0][rr][cc];
                a.U[p] = tile[buf][1][rr][cc];
                a.V[p] = tile[buf][2][rr][cc];
            }
        };
        auto load_bwd = [&](int c, int buf) {
            float ev[WLS_PER_MOVER], u[WLS_PER_MOVER], v[WLS_PER_MOVER];
#pragma unroll
            for (int i = 0; i < WLS_PER_MOVER; ++i) {
                size_t p;
                int rr, cc;
                elem(c, i, p, rr, cc);
                ev[i] = a.E[p], u[i] = a.U[p], v[i] = a.V[p];
            }
#pragma unroll
            for (int i = 0; i < WLS_PER_MOVER; ++i) {
                size_t p;
                int rr, cc;
                if (!elem(c, i, p, rr, cc)) continue;
                tile[buf][0][rr][cc] = ev[i], tile[buf][1][rr][cc] = u[i], tile[buf][2][rr][cc] = v[i];
            }
        };

        // Solver state of lane `lane`'s row, carried across chunks.  Lanes >= nl compute on stale tiles; nothing of
        // theirs is stored.
        float e = 0.0f, yu = 0.0f, yv = 0.0f, s_prev = 0.0f;

        if (!solver) load_fwd(0, 0);
        __syncthreads();
        for (int c = 0; c < chunks; ++c) {
            const int buf = c & 1;
            if (solver) {
                // the chunk goes to registers first, so the recurrence waits on no LDS access; cells past the map's
                // last column hold stale values that are computed on and not stored
                const int c0 = c * WLS_TW;
                const int len = min(WLS_TW, W - c0);
                float (*tg)[WLS_TP] = tile[buf][0];
                float (*tu)[WLS_TP] = tile[buf][1];
                float (*tv)[WLS_TP] = tile[buf][2];
                float Rv[WLS_TW], fu[WLS_TW], fv[WLS_TW];
#pragma unroll
                for (int cc = 0; cc < WLS_TW; ++cc) Rv[cc] = tg[lane][cc], fu[cc] = tu[lane][cc], fv[cc] = tv[lane][cc];
                if (a.first) {                       // d and confidence (stale without one: not used)
#pragma unroll
                    for (int cc = 0; cc < WLS_TW; ++cc) wls_planes(fu[cc], has_conf, fv[cc], a.invalid, fu[cc], fv[cc]);
                }
#pragma unroll
                for (int cc = 0; cc < WLS_TW; ++cc) {
                    if (cc < len) {
                        wls_forward(c0 + cc == 0, s_prev, Rv[cc], fu[cc], fv[cc], e, yu, yv);
                        s_prev = Rv[cc];
                        Rv[cc] = e, fu[cc] = yu, fv[cc] = yv;
                    }
                }
#pragma unroll
                for (int cc = 0; cc < WLS_TW; ++cc) tg[lane][cc] = Rv[cc], tu[lane][cc] = fu[cc], tv[lane][cc] = fv[cc];
            } else {
                if (c >= 1 && c < chunks - 1) store(c - 1, (c - 1) & 1, true);   // chunk chunks-2 stays in LDS
                if (c + 1 < chunks) load_fwd(c + 1, (c + 1) & 1);
            }
            __syncthreads();
        }
        // Back sweep: chunks chunks-1 and chunks-2 are still in their buffers.
        float xu = 0.0f, xv = 0.0f;
        for (int c = chunks - 1; c >= 0; --c) {
            const int buf = c & 1;
            if (solver) {
                const int c0 = c * WLS_TW;
                const int len = min(WLS_TW, W - c0);
                float (*te)[WLS_TP] = tile[buf][0];
                float (*tu)[WLS_TP] = tile[buf][1];
                float (*tv)[WLS_TP] = tile[buf][2];
                float ev[WLS_TW], bu[WLS_TW], bv[WLS_TW];
#pragma unroll
                for (int cc = 0; cc < WLS_TW; ++cc) ev[cc] = te[lane][cc], bu[cc] = tu[lane][cc], bv[cc] = tv[lane][cc];
#pragma unroll
                for (int cc = WLS_TW - 1; cc >= 0; --cc) {
                    if (cc < len) {
                        if (c0 + cc == W - 1) {
                            xu = bu[cc];
                            xv = bv[cc];
                        } else {
                            xu = __fadd_rn(bu[cc], __fmul_rn(ev[cc], xu));
                            xv = __fadd_rn(bv[cc], __fmul_rn(ev[cc], xv));
                        }
                        bu[cc] = xu, bv[cc] = xv;
                    }
                }
#pragma unroll
                for (int cc = 0; cc < WLS_TW; ++cc) tu[lane][cc] = bu[cc], tv[lane][cc] = bv[cc];
            } else {
                if (c + 1 < chunks) store(c + 1, (c + 1) & 1, false);
                if (c >= 1 && c - 1 < chunks - 2) load_bwd(c - 1, (c - 1) & 1);
            }
            __syncthreads();
        }
        if (!solver) store(0, 0, false);
        __syncthreads();                                 // the buffers are free for the next block of rows
    }
}

__global__ __launch_bounds__(WLS_COL_THREADS) void k_wls_cols(WlsArgs a, WlsTable tab) {
    __shared__ float rw[256];
    for (int k = threadIdx.x; k < 256; k += WLS_COL_THREADS) rw[k] = tab.range[k];
    __syncthreads();
    const int H = a.H, W = a.W;
    const size_t lines = (size_t)a.n * W;
    const float lam = a.lambda;
    for (size_t line = (size_t)blockIdx.x * WLS_COL_THREADS + threadIdx.x; line < lines;
         line += (size_t)gridDim.x * WLS_COL_THREADS) {
        const size_t m = line / W;
        const size_t col = m * H * W + (line - m * W);   // pixel (j, x) of this column at col + j * W
        // forward; the loads of steps j0 + WLS_PF .. are issued before steps j0 .. are computed (rows clamped to H-1:
        // values past the end are loaded and not used)
        float gq[WLS_PF], uq[WLS_PF], vq[WLS_PF];        // g_{j+1}, U_j, V_j of the current group
        auto load_f = [&](int j0, float (&g)[WLS_PF], float (&u)[WLS_PF], float (&v)[WLS_PF]) {
#pragma unroll
            for (int k = 0; k < WLS_PF; ++k) {
                const size_t j = (size_t)min(j0 + k, H - 1), jn = (size_t)min(j0 + k + 1, H - 1);
                g[k] = a.guide[col + jn * W];
                u[k] = a.U[col + j * W];
                v[k] = a.V[col + j * W];
            }
        };
        load_f(0, gq, uq, vq);
        float g = a.guide[col];
        float e = 0.0f, yu = 0.0f, yv = 0.0f, s_prev = 0.0f;
        for (int j0 = 0; j0 < H; j0 += WLS_PF) {
            float gn[WLS_PF], un[WLS_PF], vn[WLS_PF];
            load_f(j0 + WLS_PF, gn, un, vn);
            float Rq[WLS_PF];                            // off the recurrence: depends on the guide only
#pragma unroll
            for (int k = 0; k < WLS_PF; ++k)
                Rq[k] = j0 + k < H - 1 ? __fmul_rn(lam, rw[wls_range_index(k == 0 ? g : gq[k - 1], gq[k])]) : 0.0f;
#pragma unroll
            for (int k = 0; k < WLS_PF; ++k) {
                const int j = j0 + k;
                if (j >= H) break;
                const float R = Rq[k];
                wls_forward(j == 0, s_prev, R, uq[k], vq[k], e, yu, yv);
                const size_t p = col + (size_t)j * W;
                a.E[p] = e;
                a.U[p] = yu;
                a.V[p] = yv;
                s_prev = R;
            }
            g = gq[WLS_PF - 1];
#pragma unroll
            for (int k = 0; k < WLS_PF; ++k) gq[k] = gn[k], uq[k] = un[k], vq[k] = vn[k];
        }
        // back sweep, loads WLS_PB steps ahead going up (rows clamped to 0)
        float eq[WLS_PB], yuq[WLS_PB], yvq[WLS_PB];
        auto load_b = [&](int j0, float (&ee)[WLS_PB], float (&u)[WLS_PB], float (&v)[WLS_PB]) {
#pragma unroll
            for (int k = 0; k < WLS_PB; ++k) {
                const size_t j = (size_t)max(j0 - k, 0);
                ee[k] = a.E[col + j * W];
                u[k] = a.U[col + j * W];
                v[k] = a.V[col + j * W];
            }
        };
        load_b(H - 1, eq, yuq, yvq);
        float xu = 0.0f, xv = 0.0f;
        for (int j0 = H - 1; j0 >= 0; j0 -= WLS_PB) {
            float en[WLS_PB], un[WLS_PB], vn[WLS_PB];
            load_b(j0 - WLS_PB, en, un, vn);
#pragma unroll
            for (int k = 0; k < WLS_PB; ++k) {
                const int j = j0 - k;
                if (j < 0) break;
                if (j == H - 1) {
                    xu = yuq[k];
                    xv = yvq[k];
                } else {
                    xu = __fadd_rn(yuq[k], __fmul_rn(eq[k], xu));
                    xv = __fadd_rn(yvq[k], __fmul_rn(eq[k], xv));
                }
                const size_t p = col + (size_t)j * W;
                if (a.last) {
                    a.out[p] = wls_output(xu, xv, a.min_weight, a.invalid);
                } else {
                    a.U[p] = xu;
                    a.V[p] = xv;
                }
            }
#pragma unroll
            for (int k = 0; k < WLS_PB; ++k) eq[k] = en[k], yuq[k] = un[k], yvq[k] = vn[k];
        }
    }
}

}  // namespace smx
