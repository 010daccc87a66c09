// k_project.h -- point clouds projected into camera views as z-buffered disparity maps (smx_project_points).  The rule,
// bit for bit, is in include/stereo_mi355x.h; tests/project_ref.py restates it in NumPy.
//
// A scatter with a depth test, in three launches: the keys of every output pixel are set to "empty" (and the caller's
// offsets are clamped once into the workspace), one lane per point projects it and takes an unsigned 64-bit minimum of
// (bits(c_2) << 32) | j at every pixel of its footprint, one lane per pixel reads the winning key and recomputes the
// disparity from the winning point.  c_2 > 0, so its bit pattern orders as an unsigned integer, and the minimum of the
// keys is the nearest point, the lowest index among equals: an integer minimum is associative and commutative, so the
// result depends on neither the grid nor the scheduling.  Integer atomics only.
#pragma once
#include <climits>

#include "k_camera.h"

namespace smx {

constexpr unsigned long long PROJ_EMPTY = ~0ull;   // no key equals it: bits(c_2) < 0x7f800000 for a finite c_2

struct ProjectArgs {
    const float *points;            // [cap][3], rows of 12 bytes: 4-byte aligned only
    const int *offsets_in;          // [n+1] (the caller's)
    const float *w2c;               // [n][3][4]
    float p[16];
    float zmin, zmax, invalid;
    int radius, n, cap, H, W;
    float *disp;                    // [n][H][W]
    int *index;                     // [n][H][W] or NULL
    float *depth;                   // [n][H][W] or NULL
    // workspace
    unsigned long long *keys;       // [n][H][W]
    int *off;                       // [n+1], the offsets clamped to a non-decreasing sequence in [0, cap]
};

// What a point projects to, every operation one float32 operation in the header's order (-ffp-contract=off).
struct ProjPoint {
    float c2, d;
    int u, v;
};

__device__ __forceinline__ bool project_point(const ProjectArgs &a, const float *pt, const float *M, ProjPoint &r) {
    const float x = pt[0], y = pt[1], z = pt[2];
    const float c0 = affine_row(M, 0, x, y, z), c1 = affine_row(M, 1, x, y, z), c2 = affine_row(M, 2, x, y, z);
    if (!(isfinite(c2) && c2 > 0.0f && c2 >= a.zmin && c2 <= a.zmax)) return false;
    // affine_row(p, 0..3, c0, c1, c2), written out: as calls they change the splat kernel's device code
    const float *p = a.p;
    const float p0 = ((p[0] * c0 + p[1] * c1) + p[2] * c2) + p[3];
    const float p1 = ((p[4] * c0 + p[5] * c1) + p[6] * c2) + p[7];
    const float p2 = ((p[8] * c0 + p[9] * c1) + p[10] * c2) + p[11];
    const float p3 = ((p[12] * c0 + p[13] * c1) + p[14] * c2) + p[15];
    if (!(p3 > 0.0f)) return false;
    const float fu = nearest_pixel(p0, p3), fv = nearest_pixel(p1, p3);
    const float R = (float)a.radius;
    if (!(fu >= -R && fu <= (float)(a.W - 1) + R && fv >= -R && fv <= (float)(a.H - 1) + R)) return false;   // NaN fails
    const float d = p2 / p3;
    if (!(isfinite(d) && d != a.invalid)) return false;
    r.c2 = c2, r.d = d, r.u = (int)fu, r.v = (int)fv;
    return true;
}

// One key per thread; workgroup 0 first clamps the offsets: off[m] = min(cap, max(0, max(offsets[0..m]))), which is the
// sequence "each entry raised to the one before it (the first to 0), then lowered to the capacity", as a prefix maximum.
__global__ __launch_bounds__(256) void k_project_clear(const ProjectArgs a) {
    if (blockIdx.x == 0) {
        __shared__ int part[256];
        const int L = a.n + 1, per = (L + 255) / 256;
        const int lo = min(L, (int)threadIdx.x * per), hi = min(L, lo + per);
        int m = INT_MIN;
        for (int i = lo; i < hi; ++i) m = max(m, a.offsets_in[i]);
        part[threadIdx.x] = m;
        __syncthreads();
        for (int s = 1; s < 256; s <<= 1) {                       // Hillis-Steele inclusive maximum
            const int v = ((int)threadIdx.x >= s) ? part[threadIdx.x - s] : INT_MIN;
            __syncthreads();
            part[threadIdx.x] = max(part[threadIdx.x], v);
            __syncthreads();
        }
        int run = threadIdx.x > 0 ? part[threadIdx.x - 1] : INT_MIN;
        for (int i = lo; i < hi; ++i) {
            run = max(run, a.offsets_in[i]);
            a.off[i] = min(a.cap, max(0, run));
        }
    }
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < (size_t)a.n * a.H * a.W) a.keys[i] = PROJ_EMPTY;
}

// One lane per row of `points`.  The workgroup's first and last rows are searched in the offsets once; a lane's cloud
// lies between the two, which are the same cloud for all but a few workgroups.
__global__ __launch_bounds__(256) void k_project_splat(const ProjectArgs a) {
    const int p0 = blockIdx.x * 256;
    const int begin = a.off[0], end = a.off[a.n];
    if (begin >= end || p0 + 255 < begin || p0 >= end) return;
    __shared__ int span[2];
    if (threadIdx.x == 0) {
        span[0] = upper_index(a.off, 0, a.n, max(p0, begin));
        span[1] = upper_index(a.off, span[0], a.n, min(p0 + 255, end - 1));
    }
    __syncthreads();
    const int p = p0 + threadIdx.x;
    if (p < begin || p >= end) return;
    const int f = upper_index(a.off, span[0], span[1], p);   // no iteration where the workgroup has one cloud
    const int j = p - a.off[f];
    // The pose: three 16-byte loads whose address is the same in every lane of a wave that lies inside one cloud (one
    // request, broadcast).  P is in the kernel arguments.
    const float *Mp = a.w2c + (size_t)f * 12;
    float M[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) M[k] = Mp[k];
    ProjPoint r;
    if (!project_point(a, a.points + (size_t)p * 3, M, r)) return;
    const unsigned long long key = ((unsigned long long)__float_as_uint(r.c2) << 32) | (unsigned)j;
    unsigned long long *plane = a.keys + (size_t)f * a.H * a.W;
    const int y0 = max(r.v - a.radius, 0), y1 = min(r.v + a.radius, a.H - 1);
    const int x0 = max(r.u - a.radius, 0), x1 = min(r.u + a.radius, a.W - 1);
    for (int y = y0; y <= y1; ++y)
        for (int x = x0; x <= x1; ++x) {
            unsigned long long *k = plane + (size_t)y * a.W + x;
            // The filter.  A pixel's key only ever decreases during this launch, so whatever this plain load returns,
            // however stale, is >= the key's value at any later moment.  If our key is not below it, it is not below
            // the final minimum either and cannot be the winner: skipping it drops nothing.  If it is below it, the
            // atomic decides; a stale read can only let an atomic through that then loses.  (Measured, DESIGN.md: the
            // filter costs 6-14 % where every pixel gets about one candidate and saves 1.4x / 2.1x at radius 1 / 2.)
            if (key < *k) atomicMin(k, key);
        }
}

// One lane per output pixel: the winner's d (recomputed from its point by the same operations), j and c_2.
__global__ __launch_bounds__(256) void k_project_resolve(const ProjectArgs a) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t plane = (size_t)a.H * a.W;
    if (i >= (size_t)a.n * plane) return;
    const unsigned long long key = a.keys[i];
    float d = a.invalid, z = __builtin_nanf("");
    int j = -1;
    if (key != PROJ_EMPTY) {
        const int f = (int)(i / plane);
        j = (int)(unsigned)(key & 0xffffffffull);
        const float *Mp = a.w2c + (size_t)f * 12;
        float M[12];
#pragma unroll
        for (int k = 0; k < 12; ++k) M[k] = Mp[k];
        ProjPoint r{};
        project_point(a, a.points + ((size_t)a.off[f] + j) * 3, M, r);    // a winner passed every test in the splat
        d = r.d, z = __uint_as_float((unsigned)(key >> 32));
    }
    a.disp[i] = d;
    if (a.index) a.index[i] = j;
    if (a.depth) a.depth[i] = z;
}

}  // namespace smx
