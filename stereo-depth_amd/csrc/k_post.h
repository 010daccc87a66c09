// k_post.h -- disparity post-processing (include/stereo_mi355x.h: smx_filter_speckles, smx_fill_invalid).
//
// Speckle filter: connected-component labelling by union-find over the 4-neighbour "linked" relation, one launch per
// phase (phase boundaries are launch boundaries: no flags or hand-offs between workgroups inside a launch):
//   k_spk_local     one workgroup per SPK_T x SPK_T tile: union-find in LDS; writes each valid pixel's label = in-map
//                   index of its local root (-1 for a non-valid pixel) and the tile's size words: the final size at
//                   the root of a region that lies inside the tile (flagged SPK_CLOSED, skipped by every later
//                   phase), 0 elsewhere
//   k_spk_merge     one workgroup per tile: unions every linked pair across the tile's left and top borders in global
//                   memory (agent-scope atomicMin on parents, Playne & Hawick / Allegretti et al.), then compresses
//                   both start paths (atomicMin)
//   k_spk_flatten   every open label becomes its root
//   k_spk_count     one workgroup per tile: sizes of the open regions aggregated in an LDS hash table first (lanes of
//                   a wave with the same root summed before that), then one agent-scope atomic add per (workgroup,
//                   distinct root)
//   k_spk_finalize  out = (valid && size[root] <= max) ? invalid : in, read then written by the same thread
// Parents only ever decrease and label[p] <= p (a root is the smallest in-map index of what it has absorbed), so the
// union loop's progress and its exit rest only on the values returned by atomicMin; a stale parent read can only cost
// iterations.  Labels are in-map indices (< 2^30 for H, W <= 32768); the n maps never share a label array slot.
//
// Hole fill: k_fill_rows (one workgroup per row: nearest valid pixel on each side from a prefix max / suffix min scan of
// valid positions, the row's "had a valid pixel" flag) then k_fill_cols (rows flagged empty copy the min of their nearest
// non-empty rows above and below, as written by k_fill_rows).
#pragma once
#include "smx_common.h"

namespace smx {

constexpr int SPK_T = 32;                  // tile edge (pixels)
constexpr int SPK_THREADS = 256;           // 4 waves, SPK_T * SPK_T / SPK_THREADS = 4 pixels per thread
constexpr int SPK_HASH = 2048;             // count: LDS hash slots (>= 2x the tile's pixels: load factor <= 1/2)
constexpr int SPK_CLOSED = 1 << 30;         // label flag: the pixel's region lies inside its tile (in-map indices < 2^30)
constexpr int SPK_COUNT = (1 << 11) - 1;   // k_spk_local: low bits of cnt[] count the pixels (<= 1024) ...
constexpr int SPK_OPEN = 1 << 11;          // ... higher bits are the OPEN marks (up to 1024 adds of 1 << 11 fit in int)
constexpr int FILL_THREADS = 256;
constexpr int FILL_LDS_W = 4096;           // widest row staged in LDS (16 KB); wider rows read global memory

__device__ __forceinline__ bool post_valid(float d, float invalid) { return __builtin_isfinite(d) && d != invalid; }

__device__ __forceinline__ bool post_linked(float a, float b, float max_diff, float invalid) {
    return post_valid(a, invalid) && post_valid(b, invalid) && fabsf(a - b) <= max_diff;
}

// ---- parents in LDS (workgroup scope) ------------------------------------------------------------------------------
__device__ __forceinline__ int lds_parent(int *L, int i) {
    return __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ int lds_find(int *L, int i) {
    int p = lds_parent(L, i);
    while (p != i) {
        i = p;
        p = lds_parent(L, i);
    }
    return i;
}
__device__ __forceinline__ void lds_union(int *L, int a, int b) {
    for (;;) {
        a = lds_find(L, a);
        b = lds_find(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }      // link the larger root under the smaller index
        const int old = __hip_atomic_fetch_min(&L[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == b) return;                              // b was still a root: linked
        b = old;                                           // someone linked b first: retry from its new parent
    }
}

// ---- parents in global memory (agent scope: other workgroups write them in the same launch) ------------------------
__device__ __forceinline__ int g_parent(int *L, int i) {
    return __hip_atomic_load(&L[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int g_find(int *L, int i) {
    int p = g_parent(L, i);
    while (p != i) {
        i = p;
        p = g_parent(L, i);
    }
    return i;
}
// Points every node on the path from i to r at r (atomicMin: parents still only decrease); each returned old parent is the
// next node.  Stops where the path already leads below r (r was linked meanwhile).
__device__ __forceinline__ void g_compress(int *L, int i, int r) {
    while (i > r) {
        const int old = __hip_atomic_fetch_min(&L[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old <= r) return;
        i = old;
    }
}
__device__ __forceinline__ void g_union(int *L, int a, int b) {
    const int a0 = a, b0 = b;
    for (;;) {
        a = g_find(L, a);
        b = g_find(L, b);
        if (a == b) break;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(&L[b], a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == b) break;
        b = old;
    }
    g_compress(L, a0, a);                                  // shorter chains for the unions still to come
    g_compress(L, b0, a);
}

// blockIdx.x -> (map, tile): tiles in row-major order, SPK_T x SPK_T each; returns the map's offset, x0 / y0 = the tile's
// first row / column.
__device__ __forceinline__ size_t spk_tile(int H, int W, int &x0, int &y0) {
    const int ty = (W + SPK_T - 1) / SPK_T, tiles = ty * ((H + SPK_T - 1) / SPK_T);
    const int m = blockIdx.x / tiles, t = blockIdx.x - m * tiles;
    x0 = (t / ty) * SPK_T;
    y0 = (t % ty) * SPK_T;
    return (size_t)m * H * W;
}

// Wave-level grouping for LDS counters: fn(key, lanes, marked lanes) for every lane with key >= 0.  The first
// SPK_GROUP_ROUNDS distinct keys of the wave are summed over their lanes first (ballot) and fn runs once per group, on its
// first lane: a region covering the whole wave then costs one LDS atomic instead of 64 on one address.  Lanes left after
// that (a wave of many small regions) call fn(key, 1, mark) each, on distinct addresses mostly.  Must be reached by every
// lane of the wave.
constexpr int SPK_GROUP_ROUNDS = 2;
template <typename F>
__device__ __forceinline__ void wave_group(int key, bool mark, F fn) {
    bool pending = key >= 0;
    for (int round = 0; round < SPK_GROUP_ROUNDS; ++round) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;
        const int leader = __ffsll((long long)act) - 1;
        const int lk = __shfl(key, leader);
        const bool mine = pending && key == lk;
        const unsigned long long m = __ballot(mine), mm = __ballot(mine && mark);
        if ((int)(threadIdx.x % warpSize) == leader) fn(lk, __popcll(m), __popcll(mm));
        if (mine) pending = false;
    }
    if (pending) fn(key, 1, mark ? 1 : 0);
}

// grid.x = n * tiles (spk_tile).  label / size: [n][H][W] ints of the workspace.
// Row runs first (one thread per tile row: each pixel linked to its left neighbour takes that neighbour's parent, so every
// run is a star around its first pixel), then one union per vertical contact: a pixel skips the union with its upper
// neighbour when its left neighbour's union already joins the same two runs.  A local component none of whose pixels is
// linked to a pixel outside the tile is CLOSED: no later phase can change it, so its size is final here.  Its pixels get
// label = root | SPK_CLOSED and the root's size word the count; every later phase skips them.
__global__ __launch_bounds__(SPK_THREADS) void k_spk_local(const float *__restrict__ in, int *__restrict__ label,
                                                           int *__restrict__ size, int H, int W, float max_diff,
                                                           float invalid) {
    constexpr int N = SPK_T * SPK_T, PER = N / SPK_THREADS;
    __shared__ float v[N];
    __shared__ int L[N];
    __shared__ int cnt[N];                                 // local root: pixels | SPK_OPEN once a link leaves the tile
    int x0, y0;
    const size_t map = spk_tile(H, W, x0, y0);
    const float *M = in + map;
    for (int i = threadIdx.x; i < N; i += SPK_THREADS) {
        const int x = x0 + i / SPK_T, y = y0 + i % SPK_T;
        v[i] = (x < H && y < W) ? M[(size_t)x * W + y] : invalid;           // outside the map: non-valid
        L[i] = i;
        cnt[i] = 0;
    }
    __syncthreads();
    if (threadIdx.x < SPK_T) {
        const int r0 = threadIdx.x * SPK_T;
        for (int c = 1; c < SPK_T; ++c)
            if (post_linked(v[r0 + c], v[r0 + c - 1], max_diff, invalid)) L[r0 + c] = L[r0 + c - 1];
    }
    __syncthreads();
    for (int i = threadIdx.x + SPK_T; i < N; i += SPK_THREADS) {
        if (!post_linked(v[i], v[i - SPK_T], max_diff, invalid)) continue;
        if (i % SPK_T && post_linked(v[i], v[i - 1], max_diff, invalid) &&
            post_linked(v[i - 1], v[i - 1 - SPK_T], max_diff, invalid) &&
            post_linked(v[i - SPK_T], v[i - 1 - SPK_T], max_diff, invalid))
            continue;                                      // the left neighbour's union covers this contact
        lds_union(L, i, i - SPK_T);
    }
    __syncthreads();
    int root[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = threadIdx.x + k * SPK_THREADS;
        root[k] = -1;
        bool open = false;                                 // a link to a pixel of another tile
        if (post_valid(v[i], invalid)) {                   // false for every pixel outside the map
            const int c = i % SPK_T, x = x0 + i / SPK_T, y = y0 + c;
            root[k] = lds_find(L, i);
            if (c == 0 && y > 0) open |= post_linked(v[i], M[(size_t)x * W + y - 1], max_diff, invalid);
            if (c == SPK_T - 1 && y + 1 < W) open |= post_linked(v[i], M[(size_t)x * W + y + 1], max_diff, invalid);
            if (i < SPK_T && x > 0) open |= post_linked(v[i], M[(size_t)(x - 1) * W + y], max_diff, invalid);
            if (i >= N - SPK_T && x + 1 < H) open |= post_linked(v[i], M[(size_t)(x + 1) * W + y], max_diff, invalid);
        }
        // pixels in the low bits, one SPK_OPEN per open pixel in the high bits (only "any" matters)
        wave_group(root[k], open, [&](int r, int px, int op) { atomicAdd(&cnt[r], px + SPK_OPEN * op); });
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = threadIdx.x + k * SPK_THREADS, x = x0 + i / SPK_T, y = y0 + i % SPK_T;
        if (x >= H || y >= W) continue;
        const int r = root[k];
        int lab = -1, sz = 0;
        if (r >= 0) {
            const int c = cnt[r];
            const bool closed = (c & ~SPK_COUNT) == 0;
            lab = ((x0 + r / SPK_T) * W + (y0 + r % SPK_T)) | (closed ? SPK_CLOSED : 0);
            if (closed && r == i) sz = c;
        }
        const size_t p = map + (size_t)x * W + y;
        label[p] = lab;
        size[p] = sz;
    }
}

// grid.x = n * tiles (spk_tile), 2 * SPK_T threads: thread t < SPK_T joins row x0 + t across the tile's left border,
// thread SPK_T + t joins column y0 + t across its top border.
__global__ __launch_bounds__(2 * SPK_T) void k_spk_merge(const float *__restrict__ in, int *label, int H, int W,
                                                         float max_diff, float invalid) {
    int x0, y0;
    const size_t map = spk_tile(H, W, x0, y0);
    const int t = threadIdx.x % SPK_T;
    int p, q;                                              // in-map indices of the pair
    if (threadIdx.x < SPK_T) {
        const int x = x0 + t;
        if (y0 == 0 || x >= H) return;
        p = x * W + y0;
        q = p - 1;
    } else {
        const int y = y0 + t;
        if (x0 == 0 || y >= W) return;
        p = x0 * W + y;
        q = p - W;
    }
    const float *M = in + map;
    if (!post_linked(M[p], M[q], max_diff, invalid)) return;
    // the previous pair along the border (one row up / one column left, same two tiles) already joins both sides
    const int s = threadIdx.x < SPK_T ? W : 1;             // step back along the border
    if (t > 0 && post_linked(M[p - s], M[q - s], max_diff, invalid) && post_linked(M[p], M[p - s], max_diff, invalid) &&
        post_linked(M[q], M[q - s], max_diff, invalid))
        return;
    g_union(label + map, p, q);                           // starts from the pixels: their labels lead to the roots
}

// one thread per pixel (grid-stride); every label becomes its root.  Other threads compress paths in the same launch:
// every parent read is an agent-scope atomic load, and a value read is always an ancestor, written or not.
__global__ __launch_bounds__(SPK_THREADS) void k_spk_flatten(int *label, int H, int W, int n) {
    const size_t hw = (size_t)H * W, total = hw * n;
    for (size_t p = (size_t)blockIdx.x * SPK_THREADS + threadIdx.x; p < total; p += (size_t)gridDim.x * SPK_THREADS) {
        const int own = (int)(p % hw);
        int *Lm = label + (p - own);
        const int l = g_parent(Lm, own);
        if (l < 0 || (l & SPK_CLOSED) || l == own) continue;
        const int r = g_find(Lm, l);
        __hip_atomic_store(&Lm[own], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// grid.x = n * tiles (spk_tile).  size[root] += pixels of this tile with that root, one atomic add per distinct root.
__global__ __launch_bounds__(SPK_THREADS) void k_spk_count(const int *__restrict__ label, int *size, int H, int W) {
    __shared__ int key[SPK_HASH];
    __shared__ int cnt[SPK_HASH];
    int x0, y0;
    const size_t map = spk_tile(H, W, x0, y0);
    for (int i = threadIdx.x; i < SPK_HASH; i += SPK_THREADS) {
        key[i] = -1;
        cnt[i] = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SPK_T * SPK_T; i += SPK_THREADS) {   // uniform trip count: wave_group is reached
        const int x = x0 + i / SPK_T, y = y0 + i % SPK_T;
        int r = (x < H && y < W) ? label[map + (size_t)x * W + y] : -1;
        if (r & SPK_CLOSED) r = -1;                        // closed regions were counted by k_spk_local
        wave_group(r, false, [&](int rk, int px, int) {
            unsigned h = ((unsigned)rk * 2654435761u) >> (32 - 11);     // SPK_HASH = 2^11
            for (;;) {                                     // linear probing; at most 1024 keys in 2048 slots
                const int k = atomicCAS(&key[h], -1, rk);
                if (k == -1 || k == rk) break;
                h = (h + 1) & (SPK_HASH - 1);
            }
            atomicAdd(&cnt[h], px);
        });
    }
    __syncthreads();
    int *Sm = size + map;
    for (int i = threadIdx.x; i < SPK_HASH; i += SPK_THREADS) {
        const int k = key[i];
        if (k >= 0) __hip_atomic_fetch_add(&Sm[k], cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// one thread per pixel (grid-stride).  COPY: max_speckle_size == 0, label / size are not read.
template <bool COPY>
__global__ __launch_bounds__(SPK_THREADS) void k_spk_finalize(const float *in, float *out, const int *__restrict__ label,
                                                              const int *__restrict__ size, int H, int W, int n,
                                                              int max_size, float invalid) {
    const size_t hw = (size_t)H * W, total = hw * n;
    for (size_t p = (size_t)blockIdx.x * SPK_THREADS + threadIdx.x; p < total; p += (size_t)gridDim.x * SPK_THREADS) {
        const float d = in[p];
        bool drop = false;
        if (!COPY && post_valid(d, invalid)) {
            const size_t own = p % hw;
            drop = size[(p - own) + (label[p] & ~SPK_CLOSED)] <= max_size;
        }
        out[p] = drop ? invalid : d;
    }
}

// ---- hole fill ---------------------------------------------------------------------------------------------------
// grid.x = n * H rows.  Each thread owns one contiguous chunk of the row.  First every thread reads its chunk (LDS: the
// whole row is staged; global: the chunk's own elements) and the workgroup scans, behind a barrier, the last valid
// position of every earlier chunk (prefix max) and the first valid position of every later chunk (suffix min).  Then
// each thread writes its own chunk only: in place it re-reads only its own elements (no other thread writes them) and the
// values at valid positions, which every writer leaves as they are.  flags[row] = the row had a valid pixel.
template <bool LDS>
__global__ __launch_bounds__(FILL_THREADS) void k_fill_rows(const float *in, float *out, int *__restrict__ flags, int W,
                                                            float invalid) {
    __shared__ float row[LDS ? FILL_LDS_W : 1];
    __shared__ int lastv[FILL_THREADS], firstv[FILL_THREADS];
    const size_t base = (size_t)blockIdx.x * W;
    const float *src = LDS ? row : in + base;
    if (LDS) {
        for (int y = threadIdx.x; y < W; y += FILL_THREADS) row[y] = in[base + y];
        __syncthreads();
    }
    const int chunk = (W + FILL_THREADS - 1) / FILL_THREADS;
    const int c0 = threadIdx.x * chunk, c1 = min(W, c0 + chunk);
    int last = -1, first = W;
    for (int y = c0; y < c1; ++y)
        if (post_valid(src[y], invalid)) {
            last = y;
            if (first == W) first = y;
        }
    lastv[threadIdx.x] = last;
    firstv[threadIdx.x] = first;
    __syncthreads();
    // inclusive Hillis-Steele scans: lastv -> max over chunks <= t, firstv -> min over chunks >= t
    for (int off = 1; off < FILL_THREADS; off <<= 1) {
        const int t = threadIdx.x;
        const int a = t >= off ? lastv[t - off] : -1;
        const int b = t + off < FILL_THREADS ? firstv[t + off] : W;
        __syncthreads();
        lastv[t] = max(lastv[t], a);
        firstv[t] = min(firstv[t], b);
        __syncthreads();
    }
    if (threadIdx.x == 0) flags[blockIdx.x] = lastv[FILL_THREADS - 1] >= 0 ? 1 : 0;
    if (c0 >= c1) return;
    int left = threadIdx.x > 0 ? lastv[threadIdx.x - 1] : -1;                    // nearest valid column < c0
    const int right_end = threadIdx.x + 1 < FILL_THREADS ? firstv[threadIdx.x + 1] : W;   // nearest valid column >= c1
    const float *rd = LDS ? row : in + base;               // valid positions only, outside this chunk
    float *o = out + base;
    int run = c0;                                          // first non-valid column of the pending run
    for (int y = c0; y <= c1; ++y) {
        const int b = y < c1 ? (post_valid(src[y], invalid) ? y : -1) : (right_end < W ? right_end : -2);
        if (b == -1) continue;                             // non-valid: the run goes on
        // fill [run, y) between `left` and b (b == -2: no valid pixel to the right)
        if (run < y) {
            const bool hl = left >= 0, hr = b >= 0;
            float fv = 0.0f;
            if (hl && hr) {
                const float va = rd[left], vb = rd[b];
                fv = va <= vb ? va : vb;
            } else if (hl) {
                fv = rd[left];
            } else if (hr) {
                fv = rd[b];
            }
            for (int k = run; k < y; ++k) o[k] = (hl || hr) ? fv : src[k];
        }
        if (y < c1) {
            o[y] = src[y];
            left = y;
            run = y + 1;
        }
    }
}

// grid.x = n * H rows.  Only rows flagged empty work: r1 / r2 = nearest flagged rows above / below in the same map.
__global__ __launch_bounds__(FILL_THREADS) void k_fill_cols(float *out, const int *__restrict__ flags, int H, int W) {
    __shared__ int above[FILL_THREADS], below[FILL_THREADS];
    const int g = blockIdx.x, x = g % H;
    const int *f = flags + (g - x);
    if (f[x]) return;                                      // uniform over the workgroup
    int a = -1, b = H;
    for (int r = threadIdx.x; r < H; r += FILL_THREADS)
        if (f[r]) {
            if (r < x) a = max(a, r);
            else b = min(b, r);
        }
    above[threadIdx.x] = a;
    below[threadIdx.x] = b;
    __syncthreads();
    for (int off = FILL_THREADS / 2; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) {
            above[threadIdx.x] = max(above[threadIdx.x], above[threadIdx.x + off]);
            below[threadIdx.x] = min(below[threadIdx.x], below[threadIdx.x + off]);
        }
        __syncthreads();
    }
    const int r1 = above[0], r2 = below[0];
    if (r1 < 0 && r2 >= H) return;                         // the whole map is non-valid: left as copied
    float *o = out + (size_t)g * W;
    const float *p1 = out + (size_t)(g - x + r1) * W, *p2 = out + (size_t)(g - x + r2) * W;
    for (int y = threadIdx.x; y < W; y += FILL_THREADS) {
        float v;
        if (r1 >= 0 && r2 < H) {
            const float va = p1[y], vb = p2[y];
            v = va <= vb ? va : vb;
        } else {
            v = r1 >= 0 ? p1[y] : p2[y];
        }
        o[y] = v;
    }
}

}  // namespace smx
