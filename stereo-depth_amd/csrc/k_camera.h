// k_camera.h -- the camera and volume arithmetic the 3D kernel families share, each operation spelled once: the order of
// single float32 operations that include/stereo_mi355x.h fixes (no contraction: -ffp-contract=off).  The functions return
// values and decide nothing; every test, early return and `continue` stays in the caller.  Host and device code.
#pragma once
#include "smx_common.h"

namespace smx {

// row r of a row-major matrix with row stride 4, applied to (x, y, z, 1): ((m0*x + m1*y) + m2*z) + m3
SMX_FN float affine_row(const float *m, int r, float x, float y, float z) {
    return ((m[4 * r] * x + m[4 * r + 1] * y) + m[4 * r + 2] * z) + m[4 * r + 3];
}
// the row without its third operand, the ray of pixel (u, v): (m0*u + m1*v) + m3
SMX_FN float pixel_ray_row(const float *m, int r, float u, float v) { return (m[4 * r] * u + m[4 * r + 1] * v) + m[4 * r + 3]; }
// the rotation row on (a, b, 1), a ray's direction in the world: (m0*a + m1*b) + m2
SMX_FN float rotation_row(const float *m, int r, float a, float b) { return (m[4 * r] * a + m[4 * r + 1] * b) + m[4 * r + 2]; }

// a projection rounded to the nearest pixel: the quotient, then + 0.5f, then floorf (a NaN stays a NaN)
SMX_FN float nearest_pixel(float p, float p3) { return floorf(p / p3 + 0.5f); }

// a float colour as a byte: + 0.5f, floorf, clamped to 0..255 with fmaxf first (fmaxf(NaN, 0) = 0), converted to T at once
template <class T = unsigned> SMX_FN T colour_byte(float v) { return (T)fminf(fmaxf(floorf(v + 0.5f), 0.0f), 255.0f); }

// the plane of channel ch of image m in a planar batch of 1-channel ([n][H][W]) or 3-channel ([n][3][H][W]) images
SMX_FN size_t channel_plane(int m, int ch, int chs) { return (size_t)m * (chs == 3 ? 3 : 1) + (chs == 3 ? ch : 0); }

// the centre of voxel i along an axis with origin o and voxel size s: (float)i + 0.5f, times s, plus o
SMX_FN float voxel_centre(float o, int i, float s) { return o + ((float)i + 0.5f) * s; }
// the linear index of voxel [k][j][i] of a volume [nz][ny][nx], in size_t from the first product on
SMX_FN size_t voxel_index(int k, int j, int i, int ny, int nx) { return ((size_t)k * ny + j) * nx + i; }

// the last m in lo..hi with tab[m] <= p (tab non-decreasing on lo..hi, tab[lo] <= p); the midpoint rounds up
SMX_FN int upper_index(const int *tab, int lo, int hi, int p) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[mid] <= p) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace smx
