// k_tsdf_window.h -- a window of a TSDF volume's state as a volume of its own (smx_tsdf_window): destination voxel
// (i, j, k) takes the three state words of source voxel (x0 + i, y0 + j, z0 + k), or the empty state (all-zero bits) where
// that voxel lies outside the source grid.  The rule is in include/stereo_mi355x.h; tests/tsdf_window_ref.py restates it as
// NumPy slicing.  Shifting a volume, cropping or growing it and cutting out what a shift leaves behind are all this copy.
//
// The state is moved as 32-bit words (the colour word whole), so no float operation sees a value.  One wave per
// destination row (k, j) and four rows per workgroup: whether the source row exists and where both rows start is decided
// once per row with wave-uniform values, and a row without a source is zero stores alone.  (Waves that stay and walk
// several rows each were measured slower: DESIGN.md.)  Inside a row a lane moves one quad of 4 voxels (16 bytes) per
// array and step: the store is an aligned dwordx4 -- the quads start at the row's first 16-byte boundary, which differs
// from array to array -- and the load a dwordx4 at the 4-byte alignment that x0 leaves.
// A quad that lies wholly outside [lo, hi), the row's voxels that have a source, is stored as zeros without a load; the
// at most two quads that straddle lo or hi gather their words one by one; the up to 3 + 3 voxels before the first and
// after the last whole quad are single words.  Loads and stores carry the nontemporal hint: every byte is touched once.
// No atomics, no workspace, no LDS: the kernel is bound by the bytes it moves.
#pragma once
#include <cstddef>

#include "smx_common.h"

namespace smx {

constexpr int WIN_ARRAYS = 3;          // tsdf, weight, color
constexpr int WIN_WAVES = 4;           // waves = rows per workgroup

struct TsdfWindowArgs {
    int nx, ny, nz;                    // source dims
    int x0, y0, z0;                    // the window's first voxel in the source, any sign
    int bx, by, bz;                    // window = destination dims
    const unsigned *src[WIN_ARRAYS];   // [nz][ny][nx] words; src[2] / dst[2] NULL: no colour
    unsigned *dst[WIN_ARRAYS];         // [bz][by][bx]
};

typedef unsigned win_quad __attribute__((ext_vector_type(4)));
typedef unsigned win_quad_a4 __attribute__((ext_vector_type(4), aligned(4)));   // a source quad: x0 decides its phase

// One destination row d[0 .. bx) by one wave; s[i] is the source of d[i] and exists for lo <= i < hi only.
__device__ __forceinline__ void window_row(unsigned *__restrict__ d, const unsigned *__restrict__ s, int bx, int lo,
                                           int hi, int lane) {
    const int to_boundary = (int)((0u - (unsigned)((uintptr_t)d >> 2)) & 3u);
    const int head = to_boundary < bx ? to_boundary : bx;
    const int quads = (bx - head) >> 2;
    for (int q = lane; q < quads; q += 64) {
        const int i = head + 4 * q;
        win_quad v = {0u, 0u, 0u, 0u};
        if (i >= lo && i + 4 <= hi) {
            v = __builtin_nontemporal_load(reinterpret_cast<const win_quad_a4 *>(s + i));   // global_load_dwordx4 ... nt
        } else if (i < hi && i + 4 > lo) {                          // straddles lo or hi: at most two quads of a row
            if (i >= lo) v.x = s[i];
            if (i + 1 >= lo && i + 1 < hi) v.y = s[i + 1];
            if (i + 2 >= lo && i + 2 < hi) v.z = s[i + 2];
            if (i + 3 < hi) v.w = s[i + 3];
        }
        __builtin_nontemporal_store(v, reinterpret_cast<win_quad *>(d + i));
    }
    const int tail = head + 4 * quads;                              // [0, head) and [tail, bx): single words
    if (lane < head + (bx - tail)) {
        const int i = lane < head ? lane : tail + (lane - head);
        d[i] = (i >= lo && i < hi) ? s[i] : 0u;
    }
}

__global__ __launch_bounds__(64 * WIN_WAVES) void k_tsdf_window(const TsdfWindowArgs a) {
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned rows = (unsigned)a.by * (unsigned)a.bz;          // <= 2^24
    const unsigned r = blockIdx.x * WIN_WAVES + wave;               // this wave's row
    if (r >= rows) return;
    const unsigned k = r / (unsigned)a.by, j = r - k * (unsigned)a.by;
    const int lo = a.x0 < 0 ? -a.x0 : 0;                            // source x = x0 + i is inside the grid for lo <= i < hi
    const int hi = a.nx - a.x0 < a.bx ? a.nx - a.x0 : a.bx;
    const int sy = a.y0 + (int)j, sz = a.z0 + (int)k;
    const bool has_source = sy >= 0 && sy < a.ny && sz >= 0 && sz < a.nz && lo < hi;
    const size_t drow = (size_t)r * (size_t)a.bx;
    const ptrdiff_t srow = has_source ? ((ptrdiff_t)sz * a.ny + sy) * (ptrdiff_t)a.nx + a.x0 : 0;
#pragma unroll
    for (int t = 0; t < WIN_ARRAYS; ++t)
        if (a.dst[t])
            window_row(a.dst[t] + drow, a.src[t] + srow, a.bx, has_source ? lo : 0, has_source ? hi : 0, lane);
}

}  // namespace smx
