// k_tsdf.h -- truncated signed distance (TSDF) fusion of posed disparity maps into a dense voxel volume
// (smx_tsdf_integrate) and the ordered extraction of its zero crossings as points (smx_tsdf_extract_points).  The rules,
// bit for bit, are in include/stereo_mi355x.h; tests/tsdf_ref.py restates them in NumPy.
//
// Integration: one pass over the n*H*W pixels writes each pixel's measurement (Zm, w: NaN Zm = not accepted) and its
// colour word into the workspace; then one thread per voxel, 64 consecutive x voxels per wave, walks the n frames in
// order with the poses read as wave-uniform values.  A voxel's state is loaded when a frame first measures it, kept in
// registers across the frames and stored once at the end, only if some frame measured it.  No atomics.
//
// Extraction: the ordered compaction of k_reproject.h over the ny*nz rows of x voxels -- one workgroup per row counts
// its crossings, the shared three-launch scan (tu_reproject.hip) gives every row its first output index, one workgroup
// per row scatters the points in (voxel, axis) order.
#pragma once
#include <climits>

#include "k_camera.h"
#include "k_compact.h"

namespace smx {

struct TsdfArgs {
    int nx, ny, nz;
    float ox, oy, oz, s, tau, max_weight;
    float *tsdf, *weight;
    unsigned *color;                 // [nz][ny][nx] words R | G << 8 | B << 16, or NULL
    int n, H, W;
    const float *disp, *conf;        // [n][H][W]; conf NULL: every accepted pixel weighs 1
    float q[16], p[16];
    const float *__restrict__ pose;  // [n][3][4] world -> camera
    float min_conf, zmin, zmax, invalid;
    const void *image;               // NULL, gray [n][H][W] or RGB [n][3][H][W]
    int channels, img_f32;
    float2 *meas;                    // workspace [n*H*W]: (Zm or NaN, w)
    unsigned *pcol;                  // workspace [n*H*W]: the pixel's colour word (with a colour volume)
};

__device__ __forceinline__ unsigned tsdf_channel(const TsdfArgs &a, int m, int ch, size_t px) {
    const size_t j = channel_plane(m, ch, a.channels) * ((size_t)a.H * a.W) + px;
    return a.img_f32 ? colour_byte(((const float *)a.image)[j]) : (unsigned)((const uint8_t *)a.image)[j];
}

// one thread per pixel of the n maps: the measurement of the acceptance rule of smx_reproject_points (without X, Y),
// every step one float32 operation in the header's order
__global__ __launch_bounds__(256) void k_tsdf_pixels(const TsdfArgs a) {
    const size_t plane = (size_t)a.H * a.W, total = plane * a.n;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int m = (int)(i / plane);
    const size_t px = i - (size_t)m * plane;
    const int y = (int)(px / a.W), x = (int)(px - (size_t)y * a.W);
    const float d = a.disp[i];
    const float u = (float)x, v = (float)y;
    const float *q = a.q;
    float zm = __builtin_nanf(""), w = 1.0f;
    bool ok = isfinite(d) && d != a.invalid;
    if (ok) {
        const float zw = affine_row(q, 2, u, v, d), ww = affine_row(q, 3, u, v, d);
        ok = ww > 0.0f;
        if (ok) {
            const float z = zw / ww;
            ok = isfinite(z) && z >= a.zmin && z <= a.zmax;
            if (ok && a.conf) {
                w = a.conf[i];
                ok = w >= a.min_conf && w > 0.0f;               // a NaN confidence excludes the pixel
            }
            if (ok) zm = z;
        }
    }
    a.meas[i] = make_float2(zm, w);
    if (a.color) {
        unsigned c = 0;
        if (a.image) {
            const unsigned r = tsdf_channel(a, m, 0, px);
            c = a.channels == 3 ? r | (tsdf_channel(a, m, 1, px) << 8) | (tsdf_channel(a, m, 2, px) << 16)
                                : r | (r << 8) | (r << 16);
        }
        a.pcol[i] = c;
    }
}

// C = ((C0*W0) + (I*w)) / (W0 + w), stored as colour_byte(C), per channel of the colour words
__device__ __forceinline__ unsigned tsdf_blend_colour(unsigned c0, unsigned in, float W0, float w, float den) {
    unsigned out = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float C0 = (float)((c0 >> (8 * ch)) & 255u), I = (float)((in >> (8 * ch)) & 255u);
        out |= colour_byte(((C0 * W0) + (I * w)) / den) << (8 * ch);
    }
    return out;
}

// one thread per voxel: blockIdx.x * 64 + lane = i, blockIdx.y * 4 + wave = j, blockIdx.z = k
__global__ __launch_bounds__(256) void k_tsdf_integrate(const TsdfArgs a) {
    const int i = blockIdx.x * 64 + (threadIdx.x & 63);
    const int j = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int k = blockIdx.z;
    if (i >= a.nx || j >= a.ny) return;
    const float gx = voxel_centre(a.ox, i, a.s), gy = voxel_centre(a.oy, j, a.s), gz = voxel_centre(a.oz, k, a.s);
    const size_t vox = voxel_index(k, j, i, a.ny, a.nx);
    const float wmax = (float)(a.W - 1), hmax = (float)(a.H - 1);
    const float *P = a.p;
    float T = 0.0f, Wt = 0.0f;
    unsigned col = 0;
    bool have = false;
    for (int f = 0; f < a.n; ++f) {
        const float *M = a.pose + (size_t)f * 12;
        const float c2 = affine_row(M, 2, gx, gy, gz);
        if (!(c2 > 0.0f)) continue;
        const float c0 = affine_row(M, 0, gx, gy, gz), c1 = affine_row(M, 1, gx, gy, gz);
        const float p3 = affine_row(P, 3, c0, c1, c2);
        if (!(p3 > 0.0f)) continue;
        const float fu = nearest_pixel(affine_row(P, 0, c0, c1, c2), p3);
        const float fv = nearest_pixel(affine_row(P, 1, c0, c1, c2), p3);
        if (!(fu >= 0.0f && fu <= wmax && fv >= 0.0f && fv <= hmax)) continue;   // NaN fails
        const size_t px = ((size_t)f * a.H + (int)fv) * a.W + (int)fu;
        const float2 mw = a.meas[px];
        const float sdf = mw.x - c2;                                            // NaN Zm: not accepted
        if (!(sdf >= -a.tau)) continue;
        const float w = mw.y;
        const float t = fminf(sdf / a.tau, 1.0f);
        if (!have) {
            T = a.tsdf[vox];
            Wt = a.weight[vox];
            if (a.color) col = a.color[vox];
            have = true;
        }
        const float W0 = Wt, den = W0 + w;
        T = ((T * W0) + (t * w)) / den;
        Wt = fminf(den, a.max_weight);
        if (a.color) col = tsdf_blend_colour(col, a.pcol[px], W0, w, den);
    }
    if (have) {
        a.tsdf[vox] = T;
        a.weight[vox] = Wt;
        if (a.color) a.color[vox] = col;
    }
}

// ---- extraction -------------------------------------------------------------------------------------------------------
struct TsdfExtractArgs {
    int nx, ny, nz;
    float ox, oy, oz, s, min_weight;
    const float *tsdf, *weight;
    const unsigned *color;           // or NULL
    unsigned capacity;
    float *points, *normals;         // [capacity][3]; normals may be NULL
    uint8_t *colors;                 // [capacity][3] or NULL
    int *count;
    int *row_count, *row_offset;     // [ny*nz] each (workspace)
};

__device__ __forceinline__ bool tsdf_side_ok(const TsdfExtractArgs &a, size_t v, float &T) {
    if (!(a.weight[v] >= a.min_weight)) return false;
    T = a.tsdf[v];
    return fabsf(T) < 1.0f;                                                     // NaN fails
}

// bit a of the result: voxel (i, j, k) emits a point along axis a (x, y, z)
__device__ __forceinline__ unsigned tsdf_crossings(const TsdfExtractArgs &a, int i, int j, int k, size_t v) {
    float T0, T1;
    if (!tsdf_side_ok(a, v, T0)) return 0u;
    const bool pos = T0 >= 0.0f;
    const size_t step[3] = {1, (size_t)a.nx, (size_t)a.nx * a.ny};
    const bool inside[3] = {i + 1 < a.nx, j + 1 < a.ny, k + 1 < a.nz};
    unsigned mask = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax)
        if (inside[ax] && tsdf_side_ok(a, v + step[ax], T1) && (T1 >= 0.0f) != pos) mask |= 1u << ax;
    return mask;
}

// one workgroup (256 threads) per row r = k*ny + j: the number of crossings of the row
__global__ __launch_bounds__(256) void k_tsdf_count(const TsdfExtractArgs a) {
    const int r = blockIdx.x, j = r % a.ny, k = r / a.ny;
    __shared__ int wsum[4];
    int cnt = 0;
    for (int i = threadIdx.x; i < a.nx; i += 256)
        cnt += __popc(tsdf_crossings(a, i, j, k, (size_t)r * a.nx + i));
    const int total = block_count(cnt, wsum);
    if (threadIdx.x == 0) a.row_count[r] = total;
}

__device__ __forceinline__ size_t tsdf_clamped(int c, int d, int lim, size_t v, size_t step) {
    return c + d < 0 || c + d >= lim ? v : (d > 0 ? v + step : v - step);
}

// writes the point (normal, colour) of voxel v's crossing along axis ax to output index o
__device__ void tsdf_emit(const TsdfExtractArgs &a, int i, int j, int k, size_t v, int ax, unsigned o) {
    const size_t step[3] = {1, (size_t)a.nx, (size_t)a.nx * a.ny};
    const float T0 = a.tsdf[v], T1 = a.tsdf[v + step[ax]];
    const float t = T0 / (T0 - T1);
    float g[3] = {voxel_centre(a.ox, i, a.s), voxel_centre(a.oy, j, a.s), voxel_centre(a.oz, k, a.s)};
    g[ax] = g[ax] + t * a.s;
    float *pt = a.points + (size_t)o * 3;
    pt[0] = g[0]; pt[1] = g[1]; pt[2] = g[2];
    if (a.normals) {
        const int c[3] = {i, j, k}, lim[3] = {a.nx, a.ny, a.nz};
        float d[3];
#pragma unroll
        for (int b = 0; b < 3; ++b)
            d[b] = a.tsdf[tsdf_clamped(c[b], 1, lim[b], v, step[b])] - a.tsdf[tsdf_clamped(c[b], -1, lim[b], v, step[b])];
        const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
        float *nm = a.normals + (size_t)o * 3;
        if (len == 0.0f) {
            nm[0] = 0.0f; nm[1] = 0.0f; nm[2] = 0.0f;
        } else {
            nm[0] = d[0] / len; nm[1] = d[1] / len; nm[2] = d[2] / len;
        }
    }
    if (a.colors) {
        const unsigned cw = a.color[t <= 0.5f ? v : v + step[ax]];
        uint8_t *oc = a.colors + (size_t)o * 3;
        oc[0] = (uint8_t)(cw & 255u); oc[1] = (uint8_t)((cw >> 8) & 255u); oc[2] = (uint8_t)((cw >> 16) & 255u);
    }
}

// one workgroup per row: ordered scatter of the row's crossings; the last row also writes the total (saturated to
// INT_MAX) to count.  Output indices are unsigned: 3 * 2^30 crossings still fit.
__global__ __launch_bounds__(256) void k_tsdf_scatter(const TsdfExtractArgs a) {
    const int r = blockIdx.x, j = r % a.ny, k = r / a.ny;
    __shared__ unsigned base;
    __shared__ unsigned wcnt[4];
    if (threadIdx.x == 0) base = (unsigned)a.row_offset[r];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int x0 = 0; x0 < a.nx; x0 += 256) {
        const int i = x0 + threadIdx.x;
        const size_t v = (size_t)r * a.nx + i;
        const unsigned mask = i < a.nx ? tsdf_crossings(a, i, j, k, v) : 0u;
        const unsigned c = __popc(mask);
        unsigned incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) wcnt[wv] = incl;
        __syncthreads();
        unsigned o = base + incl - c;
        for (int w = 0; w < wv; ++w) o += wcnt[w];
#pragma unroll
        for (int ax = 0; ax < 3; ++ax)
            if ((mask >> ax) & 1u) {
                if (o < a.capacity) tsdf_emit(a, i, j, k, v, ax, o);
                ++o;
            }
        __syncthreads();
        if (threadIdx.x == 0) base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (r == a.ny * a.nz - 1 && threadIdx.x == 0) *a.count = base > (unsigned)INT_MAX ? INT_MAX : (int)base;
}

}  // namespace smx
