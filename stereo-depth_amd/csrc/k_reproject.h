// k_reproject.h -- metric 3D point clouds from disparity maps (smx_reproject_points) and their voxel-grid downsampling
// (smx_voxel_downsample).  The rules, bit for bit, are in include/stereo_mi355x.h; tests/points3d_ref.py restates them
// in NumPy.
//
// Reprojection: the ordered compaction of k_points.h extended over n*H rows -- one workgroup per row counts the pixels
// that become points (and writes the organised map), one workgroup scans the row counts (and writes the per-map
// offsets), one workgroup per row scatters the points in row-major order with wave ballots.
//
// Downsampling: a stable LSD radix sort (8-bit digits) of every map's voxel keys, each map sorted inside its own range
// [offsets[m], offsets[m+1]) so that no map bit enters the key; the key is relative to the batch's integer bounding box,
// and passes whose digit lies above the key's width are skipped on the device.  Then one thread per voxel head walks
// the voxel's points in pixel order.  Integer atomics only (bounding box, dropped counts, LDS histograms): no float
// atomics, so the output does not depend on scheduling.
#pragma once
#include <climits>

#include "k_camera.h"
#include "k_compact.h"
#include "smx_workspace.h"        // SCAN_ITEMS, SCAN_TILE, VOX_TILE, VM_COUNT: shared with the workspace layout

namespace smx {

// ---- reprojection -------------------------------------------------------------------------------------------------
struct ReprojArgs {
    const float *disp, *conf;
    const void *image;        // NULL, gray [n][H][W] or RGB [n][3][H][W]
    int channels, img_f32;    // channels 0 (no colour), 1 or 3
    float q[16];
    float min_conf, zmin, zmax, invalid;
    float *points;            // [cap][3]
    uint8_t *colors;          // [cap][3] or NULL
    int *indices;             // [cap] or NULL
    float *xyz_map;           // [n][H][W][3] or NULL
    int *offsets;             // [n+1]
    int *row_count, *row_offset;   // [n*H] each (workspace)
    int n, H, W;
};

// The point of pixel (row y, column x) of map m, if it becomes one.  Every operation is one float32 operation, in the
// order stated in the header (the unit is built with -ffp-contract=off).
__device__ __forceinline__ bool reproj_pixel(const ReprojArgs &a, size_t i, int y, int x, float &X, float &Y, float &Z) {
    const float d = a.disp[i];
    if (!(isfinite(d) && d != a.invalid)) return false;
    const float u = (float)x, v = (float)y;
    const float *q = a.q;
    const float xw = affine_row(q, 0, u, v, d), yw = affine_row(q, 1, u, v, d), zw = affine_row(q, 2, u, v, d);
    const float ww = affine_row(q, 3, u, v, d);
    if (!(ww > 0.0f)) return false;
    X = xw / ww, Y = yw / ww, Z = zw / ww;
    if (!(isfinite(X) && isfinite(Y) && isfinite(Z))) return false;
    if (!(Z >= a.zmin && Z <= a.zmax)) return false;
    if (a.conf && !(a.conf[i] >= a.min_conf)) return false;       // a NaN confidence excludes the pixel
    return true;
}

__device__ __forceinline__ uint8_t colour_at(const ReprojArgs &a, int m, int ch, int y, int x) {
    const size_t j = (channel_plane(m, ch, a.channels) * a.H + y) * a.W + x;
    return a.img_f32 ? colour_byte<uint8_t>(((const float *)a.image)[j]) : ((const uint8_t *)a.image)[j];
}

// one workgroup (256 threads) per row r = m*H + y: the number of points of the row, and the organised map
__global__ __launch_bounds__(256) void k_reproj_count(const ReprojArgs a) {
    const int r = blockIdx.x, y = r % a.H;
    __shared__ int wsum[4];
    int cnt = 0;
    const float qnan = __builtin_nanf("");
    for (int x = threadIdx.x; x < a.W; x += 256) {
        const size_t i = (size_t)r * a.W + x;
        float X, Y, Z;
        const bool ok = reproj_pixel(a, i, y, x, X, Y, Z);
        cnt += ok ? 1 : 0;
        if (a.xyz_map) {
            float *o = a.xyz_map + i * 3;
            o[0] = ok ? X : qnan; o[1] = ok ? Y : qnan; o[2] = ok ? Z : qnan;
        }
    }
    const int total = block_count(cnt, wsum);
    if (threadIdx.x == 0) a.row_count[r] = total;
}

// single workgroup: exclusive scan of the n*H row counts; offsets[m] = the offset of row m*H, offsets[n] = the total
__global__ __launch_bounds__(1024) void k_reproj_scan(const ReprojArgs a) {
    __shared__ int part[1024];
    const int rows = a.n * a.H;
    const int per = (rows + 1023) / 1024;
    const int lo = min(rows, (int)threadIdx.x * per), hi = min(rows, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += a.row_count[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {                    // Hillis-Steele inclusive scan
        const int v = (threadIdx.x >= off) ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) {
        a.row_offset[i] = run;
        if (i % a.H == 0) a.offsets[i / a.H] = run;
        run += a.row_count[i];
    }
    if (threadIdx.x == 1023) a.offsets[a.n] = part[1023];
}

// one workgroup per row: ordered scatter of the row's points (and colours, pixel indices)
__global__ __launch_bounds__(256) void k_reproj_scatter(const ReprojArgs a) {
    const int r = blockIdx.x, m = r / a.H, y = r % a.H;
    __shared__ int base;
    __shared__ int wcnt[4];
    if (threadIdx.x == 0) base = a.row_offset[r];
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int x0 = 0; x0 < a.W; x0 += 256) {                       // the slot as in k_points.h's scatter (k_compact.h)
        const int x = x0 + threadIdx.x;
        float X = 0.0f, Y = 0.0f, Z = 0.0f;
        const bool ok = x < a.W && reproj_pixel(a, (size_t)r * a.W + x, y, x, X, Y, Z);
        const unsigned long long bm = __ballot(ok);
        const int before = __popcll(bm & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wv] = __popcll(bm);
        __syncthreads();
        int woff = 0;
        for (int k = 0; k < wv; ++k) woff += wcnt[k];
        if (ok) {
            const size_t o = (size_t)(base + woff + before);
            float *pt = a.points + o * 3;
            pt[0] = X; pt[1] = Y; pt[2] = Z;
            if (a.indices) a.indices[o] = y * a.W + x;
            if (a.colors) {
                uint8_t *c = a.colors + o * 3;
                if (a.channels == 3) {
                    c[0] = colour_at(a, m, 0, y, x); c[1] = colour_at(a, m, 1, y, x); c[2] = colour_at(a, m, 2, y, x);
                } else {
                    const uint8_t g = colour_at(a, m, 0, y, x);
                    c[0] = g; c[1] = g; c[2] = g;
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) base += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

// ---- shared: exclusive scan of an int array (three launches) --------------------------------------------------------
// A launch of a skipped radix pass returns at once: gate = the key width in bits (device), pass = the pass's index.
__device__ __forceinline__ bool pass_skipped(const int *gate, int pass) { return gate && pass * 8 >= *gate; }

// exclusive scan of 256 values over the workgroup; returns this thread's prefix, *total the sum
__device__ __forceinline__ int block_exclusive_scan(int v, int *total) {
    __shared__ int wsum[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(incl, off, 64);
        if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < wv; ++k) before += wsum[k];
    *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    return before + incl - v;
}

__global__ __launch_bounds__(256) void k_scan_reduce(const int *in, long L, int *block_sums, const int *gate, int pass) {
    if (pass_skipped(gate, pass)) return;
    const long lo = (long)blockIdx.x * SCAN_TILE;
    int s = 0;
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const long i = lo + (long)k * 256 + threadIdx.x;
        if (i < L) s += in[i];
    }
    int total;
    (void)block_exclusive_scan(s, &total);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = total;
}

// single workgroup: exclusive scan of the nb block sums in place
__global__ __launch_bounds__(1024) void k_scan_top(int *block_sums, int nb, const int *gate, int pass) {
    if (pass_skipped(gate, pass)) return;
    __shared__ int part[1024];
    const int per = (nb + 1023) / 1024;
    const int lo = min(nb, (int)threadIdx.x * per), hi = min(nb, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += block_sums[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const int v = (threadIdx.x >= off) ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int run = part[threadIdx.x] - s;
    for (int i = lo; i < hi; ++i) { const int c = block_sums[i]; block_sums[i] = run; run += c; }
}

__global__ __launch_bounds__(256) void k_scan_down(const int *in, int *out, long L, const int *block_sums,
                                                   const int *gate, int pass) {
    if (pass_skipped(gate, pass)) return;
    const long lo = (long)blockIdx.x * SCAN_TILE + (long)threadIdx.x * SCAN_ITEMS;   // 16 consecutive per thread
    int v[SCAN_ITEMS];
    int s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) { v[k] = (lo + k < L) ? in[lo + k] : 0; s += v[k]; }
    int total;
    int run = block_sums[blockIdx.x] + block_exclusive_scan(s, &total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k)
        if (lo + k < L) { out[lo + k] = run; run += v[k]; }
}

// ---- voxel downsampling ----------------------------------------------------------------------------------------------
constexpr float VOX_LIMIT = 1048576.0f;   // kept iff -2^20 <= index < 2^20 on every axis
// meta[VM_COUNT]: the device-side state of one call
enum { VM_MINX = 0, VM_MINY, VM_MINZ, VM_MAXX, VM_MAXY, VM_MAXZ, VM_KEY_BITS, VM_FLAG_SHIFT, VM_TILES };

struct VoxArgs {
    const float *points;            // [cap][3]
    const uint8_t *colors;          // [cap][3] or NULL
    const int *offsets_in;          // [n+1] (the caller's)
    float voxel_size;
    int min_points, n, cap;
    float *out_points;              // [cap][3]
    uint8_t *out_colors;            // [cap][3] or NULL
    int *out_counts;                // [cap]
    int *out_offsets, *dropped;     // [n+1], [n]
    // workspace
    unsigned long long *keys[2];
    int *vals[2];
    int *counts, *counts_scan;      // [max_tiles * 256]
    int *flag, *pos, *vcnt;         // [cap + 1]
    int *block_sums;
    int *off, *tile_base, *meta;    // [n+1], [n+1], [VM_COUNT]
};

__device__ __forceinline__ bool vox_index(const float *pt, float vs, int &ix, int &iy, int &iz) {
    const float fx = floorf(pt[0] / vs), fy = floorf(pt[1] / vs), fz = floorf(pt[2] / vs);
    if (!(fx >= -VOX_LIMIT && fx < VOX_LIMIT && fy >= -VOX_LIMIT && fy < VOX_LIMIT && fz >= -VOX_LIMIT && fz < VOX_LIMIT))
        return false;                                               // NaN fails too
    ix = (int)fx, iy = (int)fy, iz = (int)fz;
    return true;
}

__device__ __forceinline__ int bit_width(int range) { return range <= 0 ? 0 : 32 - __clz(range); }

// single workgroup: the caller's offsets clamped to a non-decreasing sequence in [0, cap], the tile bases, the bounding
// box's start values, dropped[] = 0
__global__ __launch_bounds__(256) void k_vox_prep(const VoxArgs a) {
    for (int m = threadIdx.x; m < a.n; m += 256) a.dropped[m] = 0;
    if (threadIdx.x != 0) return;
    int prev = 0, tiles = 0;
    for (int m = 0; m <= a.n; ++m) {
        const int o = min(max(a.offsets_in[m], prev), a.cap);
        if (m > 0) tiles += (o - prev + VOX_TILE - 1) / VOX_TILE;
        a.off[m] = o;
        a.tile_base[m] = tiles;
        prev = o;
    }
    a.meta[VM_TILES] = tiles;
    a.meta[VM_MINX] = a.meta[VM_MINY] = a.meta[VM_MINZ] = INT_MAX;
    a.meta[VM_MAXX] = a.meta[VM_MAXY] = a.meta[VM_MAXZ] = INT_MIN;
}

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}

// Adds v to arr[m] for every lane of a full wave (m < 0 where v == 0): one atomic per wave when the lanes' maps agree,
// so that millions of points do not queue on a handful of addresses.
__device__ __forceinline__ void wave_add_to_map(int *arr, int m, int v) {
    const int m0 = wave_max(m);
    if (__ballot(v != 0 && m != m0) == 0ull) {
        int s = v;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if ((threadIdx.x & 63) == 0 && s != 0) atomicAdd(&arr[m0], s);
    } else if (v != 0) {
        atomicAdd(&arr[m], v);
    }
}

constexpr int VOX_BBOX_BLOCKS = 1024;

// grid-stride over the points (at most VOX_BBOX_BLOCKS workgroups): the integer bounding box of the kept voxel indices,
// reduced per workgroup before six atomics; out-of-range points counted as dropped
__global__ __launch_bounds__(256) void k_vox_bbox(const VoxArgs a) {
    const int lo = a.off[0], hi = a.off[a.n];
    int ix = INT_MAX, iy = INT_MAX, iz = INT_MAX, jx = INT_MIN, jy = INT_MIN, jz = INT_MIN;
    const int stride = gridDim.x * 256;
    for (int base = blockIdx.x * 256; base < hi; base += stride) {        // uniform trip count: full waves below
        const int p = base + threadIdx.x;
        int m = -1, drop = 0;
        if (p >= lo && p < hi) {
            int x, y, z;
            if (vox_index(a.points + (size_t)p * 3, a.voxel_size, x, y, z)) {
                ix = min(ix, x), iy = min(iy, y), iz = min(iz, z);
                jx = max(jx, x), jy = max(jy, y), jz = max(jz, z);
            } else {
                m = upper_index(a.off, 0, a.n, p), drop = 1;
            }
        }
        wave_add_to_map(a.dropped, m, drop);
    }
    ix = wave_min(ix), iy = wave_min(iy), iz = wave_min(iz);
    jx = wave_max(jx), jy = wave_max(jy), jz = wave_max(jz);
    __shared__ int box[4][6];
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        box[wv][0] = ix, box[wv][1] = iy, box[wv][2] = iz, box[wv][3] = jx, box[wv][4] = jy, box[wv][5] = jz;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        int v = box[0][k];
        for (int w = 1; w < 4; ++w) v = k < 3 ? min(v, box[w][k]) : max(v, box[w][k]);
        if (k < 3 ? v != INT_MAX : v != INT_MIN) {
            if (k < 3) atomicMin(&a.meta[VM_MINX + k], v);
            else atomicMax(&a.meta[VM_MINX + k], v);
        }
    }
}

// one thread per point: key = (dropped flag, ix - min x, iy - min y, iz - min z), ascending (ix, iy, iz); payload = p
__global__ __launch_bounds__(256) void k_vox_keys(const VoxArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int *mt = a.meta;
    const bool any = mt[VM_MINX] != INT_MAX;
    const int bx = any ? bit_width(mt[VM_MAXX] - mt[VM_MINX]) : 0;
    const int by = any ? bit_width(mt[VM_MAXY] - mt[VM_MINY]) : 0;
    const int bz = any ? bit_width(mt[VM_MAXZ] - mt[VM_MINZ]) : 0;
    const int shift = bx + by + bz;                                  // <= 63
    if (p == 0) { a.meta[VM_FLAG_SHIFT] = shift; a.meta[VM_KEY_BITS] = shift + 1; }
    if (p < a.off[0] || p >= a.off[a.n]) return;
    int x, y, z;
    unsigned long long key;
    if (vox_index(a.points + (size_t)p * 3, a.voxel_size, x, y, z))
        key = ((unsigned long long)(unsigned)(x - mt[VM_MINX]) << (by + bz)) |
              ((unsigned long long)(unsigned)(y - mt[VM_MINY]) << bz) | (unsigned long long)(unsigned)(z - mt[VM_MINZ]);
    else
        key = 1ull << shift;
    a.keys[0][p] = key;
    a.vals[0][p] = p;
}

// The tile of workgroup `tile`: its map, its index inside the map, the map's tile count and its point range.
struct VoxTile { int m, t, tiles, lo, hi; };
__device__ __forceinline__ VoxTile vox_tile(const VoxArgs &a, int tile) {
    VoxTile r;
    r.m = upper_index(a.tile_base, 0, a.n, tile);                   // the last map starting at or before it
    r.t = tile - a.tile_base[r.m];
    r.tiles = a.tile_base[r.m + 1] - a.tile_base[r.m];
    r.lo = a.off[r.m] + r.t * VOX_TILE;
    r.hi = min(r.lo + VOX_TILE, a.off[r.m + 1]);
    return r;
}

// one workgroup per tile: digit histogram, stored map-major then digit-major then tile so that one exclusive scan of
// the whole array gives every (map, digit, tile) its first destination relative to off[0]
__global__ __launch_bounds__(256) void k_vox_hist(const VoxArgs a, int pass) {
    if (pass * 8 >= a.meta[VM_KEY_BITS] || (int)blockIdx.x >= a.meta[VM_TILES]) return;
    const VoxTile tl = vox_tile(a, blockIdx.x);
    const unsigned long long *src = a.keys[pass & 1];
    __shared__ int h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    for (int p = tl.lo + threadIdx.x; p < tl.hi; p += 256) atomicAdd(&h[(int)((src[p] >> (pass * 8)) & 255ull)], 1);
    __syncthreads();
    a.counts[(size_t)a.tile_base[tl.m] * 256 + (size_t)threadIdx.x * tl.tiles + tl.t] = h[threadIdx.x];
}

// one workgroup per tile: stable scatter; the rank of a point among the equal digits before it in its wave comes from
// eight ballots, the waves and sub-tiles before it from LDS counts
__global__ __launch_bounds__(256) void k_vox_scatter(const VoxArgs a, int pass) {
    if (pass * 8 >= a.meta[VM_KEY_BITS] || (int)blockIdx.x >= a.meta[VM_TILES]) return;
    const VoxTile tl = vox_tile(a, blockIdx.x);
    const unsigned long long *sk = a.keys[pass & 1];
    const int *sv = a.vals[pass & 1];
    unsigned long long *dk = a.keys[(pass + 1) & 1];
    int *dv = a.vals[(pass + 1) & 1];
    __shared__ int base[256];
    __shared__ int wcnt[4][256];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    base[threadIdx.x] = a.off[0] + a.counts_scan[(size_t)a.tile_base[tl.m] * 256 + (size_t)threadIdx.x * tl.tiles + tl.t];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int p0 = tl.lo; p0 < tl.hi; p0 += 256) {
        const int p = p0 + threadIdx.x;
        const bool ok = p < tl.hi;
        const unsigned long long key = ok ? sk[p] : 0ull;
        const int val = ok ? sv[p] : 0;
        const int d = (int)((key >> (pass * 8)) & 255ull);
        for (int k = 0; k < 4; ++k) wcnt[wv][lane + 64 * k] = 0;
        unsigned long long same = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long bal = __ballot((d >> b) & 1);
            same &= ((d >> b) & 1) ? bal : ~bal;
        }
        const int rank = __popcll(same & lt), group = __popcll(same);
        __syncthreads();
        if (ok && rank == group - 1) wcnt[wv][d] = group;
        __syncthreads();
        if (ok) {
            int dst = base[d] + rank;
            for (int k = 0; k < wv; ++k) dst += wcnt[k][d];
            dk[dst] = key;
            dv[dst] = val;
        }
        __syncthreads();
        base[threadIdx.x] += wcnt[0][threadIdx.x] + wcnt[1][threadIdx.x] + wcnt[2][threadIdx.x] + wcnt[3][threadIdx.x];
        __syncthreads();
    }
}

// one thread per sorted position p in [0, cap]: flag[p] = 1 at the head of a kept voxel, vcnt[p] its point count;
// voxels below min_points add their points to dropped[]
__global__ __launch_bounds__(256) void k_vox_heads(const VoxArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;                 // every lane runs to the end (wave_add_to_map)
    int fl = 0, cnt = 0, m = -1, drop = 0;
    if (p >= a.off[0] && p < a.off[a.n]) {
        const int npass = (a.meta[VM_KEY_BITS] + 7) / 8;
        const unsigned long long *key = a.keys[npass & 1];
        const int mp = upper_index(a.off, 0, a.n, p);
        const unsigned long long k = key[p];
        const bool head = p == a.off[mp] || key[p - 1] != k;
        if (head && !((k >> a.meta[VM_FLAG_SHIFT]) & 1ull)) {
            const int end = a.off[mp + 1];
            int e = p + 1;
            while (e < end && key[e] == k) ++e;
            cnt = e - p;
            if (cnt >= a.min_points) fl = 1;
            else m = mp, drop = cnt;
        }
    }
    wave_add_to_map(a.dropped, m, drop);
    if (p > a.cap) return;
    a.flag[p] = fl;
    a.vcnt[p] = cnt;
}

// one thread per sorted position: the kept voxel heads write their centroid, mean colour and count; threads 0..n write
// the output offsets.  The centroid's sum: sequential within chunks of 64 points (pixel order), then sequential over the
// chunk sums; divided by (float)cnt.
__global__ __launch_bounds__(256) void k_vox_reduce(const VoxArgs a) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p <= a.n) a.out_offsets[p] = a.pos[a.off[p]];
    if (p >= a.cap || !a.flag[p]) return;
    const int npass = (a.meta[VM_KEY_BITS] + 7) / 8;
    const int *idx = a.vals[npass & 1] + p;
    const int cnt = a.vcnt[p], o = a.pos[p];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    unsigned long long cr = 0, cg = 0, cb = 0;
    for (int c0 = 0; c0 < cnt; c0 += 64) {
        const int c1 = min(cnt, c0 + 64);
        const float *q = a.points + (size_t)idx[c0] * 3;
        float x = q[0], y = q[1], z = q[2];
        for (int j = c0 + 1; j < c1; ++j) {
            const float *r = a.points + (size_t)idx[j] * 3;
            x += r[0]; y += r[1]; z += r[2];
        }
        if (c0 == 0) sx = x, sy = y, sz = z;
        else sx += x, sy += y, sz += z;
    }
    if (a.colors)
        for (int j = 0; j < cnt; ++j) {
            const uint8_t *c = a.colors + (size_t)idx[j] * 3;
            cr += c[0]; cg += c[1]; cb += c[2];
        }
    const float fc = (float)cnt;
    float *op = a.out_points + (size_t)o * 3;
    op[0] = sx / fc; op[1] = sy / fc; op[2] = sz / fc;
    if (a.out_colors) {
        const unsigned long long h = (unsigned long long)(cnt / 2), uc = (unsigned long long)cnt;
        uint8_t *oc = a.out_colors + (size_t)o * 3;
        oc[0] = (uint8_t)((cr + h) / uc); oc[1] = (uint8_t)((cg + h) / uc); oc[2] = (uint8_t)((cb + h) / uc);
    }
    a.out_counts[o] = cnt;
}

}  // namespace smx
