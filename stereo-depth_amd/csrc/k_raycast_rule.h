// k_raycast_rule.h -- the rule of smx_tsdf_raycast (include/stereo_mi355x.h) for one pixel: the march along its ray with
// the exact jumps k_raycast.h explains, then the outputs.  Plain C++ over the kernel's arguments, compiled for the
// device by k_raycast.h and for the host by tests/raycast_march_harness.cpp, which marches on the CPU.
#pragma once
#include "k_camera.h"

namespace smx {

struct RaycastArgs {
    int nx, ny, nz;
    int bx, by, bz;                  // bricks per axis: ceil(n_a / 8)
    float ox, oy, oz, s, min_weight;
    const float *__restrict__ tsdf, *__restrict__ weight;
    const unsigned *__restrict__ color;   // or NULL
    int n, H, W, M;
    float q[16];
    const float *__restrict__ pose;  // [n][3][4] camera -> world
    float step, zmin, invalid;
    float *disp, *depth, *normals, *out_weight;   // all but disp may be NULL
    uint8_t *colors;                 // or NULL
    uint8_t *flags, *occ;            // workspace [bz][by][bx] each: the bricks' own flags, and what the march reads
};

constexpr unsigned RC_ANY = 1u;      // a brick's byte: some voxel has weight >= min_weight;
constexpr unsigned RC_FREE = 2u;     // all have, with tsdf == 1.0f (in occ: in the brick's upper neighbours too)

struct RcRay {
    float e[3], dw[3];
};

// g_a and f_a of the point at p; true iff it is in bounds
SMX_FN bool rc_cell(const RaycastArgs &a, const float p[3], float g[3], float f[3]) {
    g[0] = (p[0] - a.ox) / a.s - 0.5f;
    g[1] = (p[1] - a.oy) / a.s - 0.5f;
    g[2] = (p[2] - a.oz) / a.s - 0.5f;
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = floorf(g[c]);
    return f[0] >= 0.0f && f[0] <= (float)(a.nx - 2) && f[1] >= 0.0f && f[1] <= (float)(a.ny - 2) && f[2] >= 0.0f &&
           f[2] <= (float)(a.nz - 2);                                // NaN fails
}

SMX_FN void rc_point(const RcRay &r, float lam, float p[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = r.e[c] + r.dw[c] * lam;
}

SMX_FN float rc_lam(const RaycastArgs &a, int m) { return a.zmin + (float)m * a.step; }

SMX_FN float rc_lerp(float x, float y, float t) { return x + (y - x) * t; }

SMX_FN void rc_corners(const float *__restrict__ v, size_t base, size_t sy, size_t sz, float c[8]) {
    c[0] = v[base], c[1] = v[base + 1], c[2] = v[base + sy], c[3] = v[base + sy + 1];
    c[4] = v[base + sz], c[5] = v[base + sz + 1], c[6] = v[base + sz + sy], c[7] = v[base + sz + sy + 1];
}

SMX_FN float rc_trilinear(const float c[8], float tx, float ty, float tz) {
    const float c00 = rc_lerp(c[0], c[1], tx), c10 = rc_lerp(c[2], c[3], tx);
    const float c01 = rc_lerp(c[4], c[5], tx), c11 = rc_lerp(c[6], c[7], tx);
    return rc_lerp(rc_lerp(c00, c10, ty), rc_lerp(c01, c11, ty), tz);
}

// Tri(p) for a point in bounds (g, f: rc_cell's)
SMX_FN float rc_tri(const RaycastArgs &a, const float g[3], const float f[3]) {
    const size_t sy = (size_t)a.nx, sz = (size_t)a.nx * a.ny;
    const size_t base = (size_t)(int)f[2] * sz + (size_t)(int)f[1] * sy + (size_t)(int)f[0];
    float c[8];
    rc_corners(a.tsdf, base, sy, sz, c);
    return rc_trilinear(c, g[0] - f[0], g[1] - f[1], g[2] - f[2]);
}

// the estimate of a jump: how many further samples stay where sample m is -- in its brick (inb), or else beyond the
// faces of the box it lies beyond.  r_a: voxels per sample along a; left: the samples after m.
SMX_FN int rc_jump_estimate(const RaycastArgs &a, const float g[3], const float f[3], const float r[3], bool inb,
                            int left) {
    const float lim[3] = {(float)(a.nx - 2), (float)(a.ny - 2), (float)(a.nz - 2)};
    float k = inb ? (float)left : 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (inb) {                                                    // leaves the brick on the first axis to run out
            const float b0 = floorf(f[c] * 0.125f) * 8.0f;
            const float d = r[c] > 0.0f ? (b0 + 8.0f) - g[c] : g[c] - b0;
            if (r[c] != 0.0f) k = fminf(k, d / fabsf(r[c]));
        } else if (f[c] < 0.0f && r[c] > 0.0f) {                      // enters the box on the last axis to arrive
            k = fmaxf(k, -g[c] / r[c]);
        } else if (f[c] > lim[c] && r[c] < 0.0f) {
            k = fmaxf(k, (g[c] - (lim[c] + 1.0f)) / -r[c]);
        }
    }
    k = floorf(k - 0.01f);                                            // a sample short rather than one too far
    return k >= 1.0f ? (int)fminf(k, (float)left) : 0;                // NaN: no jump
}

// one pixel of one view: the march, then the outputs
SMX_FN void rc_pixel(const RaycastArgs &a, int px, int py, int view) {
    const float *q = a.q;
    const float *__restrict__ M = a.pose + (size_t)view * 12;
    const float u = (float)px, v = (float)py;
    const float xp = pixel_ray_row(q, 0, u, v), yp = pixel_ray_row(q, 1, u, v), zp = pixel_ray_row(q, 2, u, v);
    const size_t sy = (size_t)a.nx, sz = (size_t)a.nx * a.ny;
    const float lim[3] = {(float)(a.nx - 2), (float)(a.ny - 2), (float)(a.nz - 2)};
    RcRay ray = {};
    bool hit = false;
    float lam_hit = 0.0f;
    if (zp > 0.0f) {
        const float rx = xp / zp, ry = yp / zp;
        float r[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            ray.dw[c] = rotation_row(M, c, rx, ry);
            ray.e[c] = M[4 * c + 3];
            r[c] = ray.dw[c] / a.s * a.step;                          // estimate only
        }
        bool pv = false;
        float pT = 0.0f;
        int m = 0;
        while (m < a.M) {
            float p[3], g[3], f[3];
            rc_point(ray, rc_lam(a, m), p);
            const bool inb = rc_cell(a, p, g, f);
            bool valid = false, jump = !inb;
            float T = 0.0f;
            if (inb) {
                const int ix = (int)f[0], iy = (int)f[1], iz = (int)f[2];
                const unsigned brick = a.occ[((size_t)(iz >> 3) * a.by + (iy >> 3)) * a.bx + (ix >> 3)];
                jump = brick != RC_ANY;                               // empty or free: nothing to load
                if (brick & RC_FREE) {
                    valid = true, T = 1.0f;
                } else if (brick) {
                    const size_t base = (size_t)iz * sz + (size_t)iy * sy + (size_t)ix;
                    float w[8], c[8];
                    rc_corners(a.weight, base, sy, sz, w);
                    rc_corners(a.tsdf, base, sy, sz, c);
                    valid = true;
#pragma unroll
                    for (int k = 0; k < 8; ++k) valid &= w[k] >= a.min_weight;
                    T = rc_trilinear(c, g[0] - f[0], g[1] - f[1], g[2] - f[2]);
                }
            } else {
                bool gone = false;                                    // beyond a face the ray moves away from
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    gone |= (f[c] < 0.0f && ray.dw[c] <= 0.0f) || (f[c] > lim[c] && ray.dw[c] >= 0.0f);
                if (gone) break;
            }
            if (valid && T < 0.0f) {
                hit = pv && pT >= 0.0f && pT < 1.0f;
                if (hit) lam_hit = rc_lam(a, m - 1) + a.step * (pT / (pT - T));
                break;
            }
            pv = valid, pT = T;
            int next = m + 1;
            if (jump) {                                               // the samples jumped over leave pv and pT as they are
                const int k = rc_jump_estimate(a, g, f, r, inb, a.M - 1 - m);
                if (k >= 1) {
                    float p2[3], g2[3], f2[3];
                    rc_point(ray, rc_lam(a, m + k), p2);
                    const bool inb2 = rc_cell(a, p2, g2, f2);
                    bool same;
                    if (inb) {                                        // still the same (empty or free) brick
                        same = inb2 && ((int)f2[0] >> 3) == ((int)f[0] >> 3) && ((int)f2[1] >> 3) == ((int)f[1] >> 3) &&
                               ((int)f2[2] >> 3) == ((int)f[2] >> 3);
                    } else {                                          // still beyond one and the same face
                        same = false;
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            same |= (f[c] < 0.0f && f2[c] < 0.0f) || (f[c] > lim[c] && f2[c] > lim[c]);
                    }
                    if (same) next = m + k + 1;
                }
            }
            m = next;
        }
    }
    const size_t plane = (size_t)a.H * a.W;
    const size_t o = (size_t)view * plane + (size_t)py * a.W + px;
    const size_t o3 = (size_t)view * 3 * plane + (size_t)py * a.W + px;
    a.disp[o] = hit ? (zp / lam_hit - q[15]) / q[14] : a.invalid;
    if (a.depth) a.depth[o] = hit ? lam_hit : __builtin_nanf("");
    if (!a.normals && !a.colors && !a.out_weight) return;
    float nrm[3] = {0.0f, 0.0f, 0.0f}, wgt = 0.0f;
    unsigned cw = 0;
    if (hit) {
        float ps[3], g[3], f[3];
        rc_point(ray, lam_hit, ps);
        if (a.normals) {
            float d[3];
            bool ok = true;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float pp[3] = {ps[0], ps[1], ps[2]}, pm[3] = {ps[0], ps[1], ps[2]};
                pp[c] = ps[c] + a.s;
                pm[c] = ps[c] - a.s;
                float hi = 0.0f, lo = 0.0f;
                if (rc_cell(a, pp, g, f)) hi = rc_tri(a, g, f);
                else ok = false;
                if (rc_cell(a, pm, g, f)) lo = rc_tri(a, g, f);
                else ok = false;
                d[c] = hi - lo;
            }
            const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
            if (ok && len != 0.0f) nrm[0] = d[0] / len, nrm[1] = d[1] / len, nrm[2] = d[2] / len;
        }
        if (a.colors || a.out_weight) {
            rc_cell(a, ps, g, f);
            const int ix = (int)fminf(fmaxf(floorf(g[0] + 0.5f), 0.0f), (float)(a.nx - 1));   // fmaxf(NaN, 0) = 0
            const int iy = (int)fminf(fmaxf(floorf(g[1] + 0.5f), 0.0f), (float)(a.ny - 1));
            const int iz = (int)fminf(fmaxf(floorf(g[2] + 0.5f), 0.0f), (float)(a.nz - 1));
            const size_t vox = (size_t)iz * sz + (size_t)iy * sy + (size_t)ix;
            if (a.colors) cw = a.color[vox];
            wgt = a.weight[vox];
        }
    }
    if (a.normals) a.normals[o3] = nrm[0], a.normals[o3 + plane] = nrm[1], a.normals[o3 + 2 * plane] = nrm[2];
    if (a.colors) {
        a.colors[o3] = (uint8_t)(cw & 255u);
        a.colors[o3 + plane] = (uint8_t)((cw >> 8) & 255u);
        a.colors[o3 + 2 * plane] = (uint8_t)((cw >> 16) & 255u);
    }
    if (a.out_weight) a.out_weight[o] = wgt;
}

}  // namespace smx
