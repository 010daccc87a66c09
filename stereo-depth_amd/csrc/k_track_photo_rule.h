// k_track_photo_rule.h -- the rule of smx_track_camera_photometric (include/stereo_mi355x.h) as plain C++ over the
// kernels' arguments: a pixel's geometric terms by k_track_rule.h's trk_pixel as it is, then its photometric terms, and
// the begin and the end of an iteration around trk_begin and trk_finish.  Compiled for the device by k_track_photo.h and
// for the host by tests/track_photo_rule_harness.cpp, which runs whole schedules on the CPU.
#pragma once
#include "k_track_rule.h"

namespace smx {

// slots of a pixel's sums: 0..29 the joint system's terms and 30 the accepted pixels, laid out as trk_pixel and
// trk_finish expect them; then the photometric sums
constexpr int TRKP_WEE = TRK_SLOTS - 1, TRKP_W = TRK_SLOTS, TRKP_COUNT = TRK_SLOTS + 1;
static_assert(TRKP_WEE == TRK_TERMS + 1 && TRKP_COUNT == TRKP_SLOTS - 1, "the photometric sums follow the accepted count");

struct TrackPhotoArgs {
    TrackArgs g;                                                     // sums: [n][TRKP_TERMS]; the partials hold TRKP_SLOTS
    const float *__restrict__ frame_int, *__restrict__ model_int;    // [n][H][W], [n][Hm][Wm]
    float weight, max_diff;                                          // lambda, max_intensity_difference
    int *pinfo;                                                      // [n][2], may be NULL
    float *prms;                                                     // [n], may be NULL
};

// Adds the terms of pixel (px, py) of frame f at the pose T to acc: the geometric ones, and after them, if the pixel was
// a geometric inlier, the photometric ones.  The values the two parts share (p, u, w) are evaluated again, by calls of
// the functions of k_camera.h that trk_pixel calls, on the same operands (keeping them across trk_pixel instead would be
// this kernel's register decision).
SMX_FN void trkp_pixel(const TrackPhotoArgs &pa, const float *T, int f, int px, int py, double acc[TRKP_SLOTS]) {
    const TrackArgs &a = pa.g;
    const double inliers = acc[29];
    trk_pixel(a, T, f, px, py, acc);
    if (acc[29] == inliers) return;                                   // counts stay far below 2^53: exact
    const size_t i = ((size_t)f * a.H + py) * a.W + px;
    const float d = a.disp[i];
    const float u = (float)px, v = (float)py;
    const float *q = a.q;
    const float ww = affine_row(q, 3, u, v, d), Z = affine_row(q, 2, u, v, d) / ww;
    const float w = a.conf ? a.conf[i] : 1.0f;
    const float X = affine_row(q, 0, u, v, d) / ww, Y = affine_row(q, 1, u, v, d) / ww;
    const float p[3] = {affine_row(T, 0, X, Y, Z), affine_row(T, 1, X, Y, Z), affine_row(T, 2, X, Y, Z)};
    const float *Mw = a.w2c + (size_t)f * 12;
    const float c[3] = {affine_row(Mw, 0, p[0], p[1], p[2]), affine_row(Mw, 1, p[0], p[1], p[2]),
                        affine_row(Mw, 2, p[0], p[1], p[2])};
    const float *P = a.pm;
    const float u3 = affine_row(P, 3, c[0], c[1], c[2]);
    const float u0 = affine_row(P, 0, c[0], c[1], c[2]), u1 = affine_row(P, 1, c[0], c[1], c[2]);
    const float x = u0 / u3, y = u1 / u3;
    const float x0 = floorf(x), y0 = floorf(y);
    if (!(x0 >= 0.0f && x0 <= (float)(a.Wm - 2) && y0 >= 0.0f && y0 <= (float)(a.Hm - 2))) return;    // NaN fails
    const size_t plane = (size_t)a.Hm * a.Wm;
    const size_t m = (size_t)f * plane + (size_t)(int)y0 * a.Wm + (size_t)(int)x0;
    const float z00 = a.depth[m], z10 = a.depth[m + 1], z01 = a.depth[m + a.Wm], z11 = a.depth[m + a.Wm + 1];
    if (!(std::isfinite(z00) && z00 > 0.0f && std::isfinite(z10) && z10 > 0.0f && std::isfinite(z01) && z01 > 0.0f &&
          std::isfinite(z11) && z11 > 0.0f))
        return;
    const float I00 = pa.model_int[m], I10 = pa.model_int[m + 1], I01 = pa.model_int[m + a.Wm];
    const float I11 = pa.model_int[m + a.Wm + 1];
    if (!(std::isfinite(I00) && std::isfinite(I10) && std::isfinite(I01) && std::isfinite(I11))) return;
    const float ax = x - x0, ay = y - y0, bx = 1.0f - ax, by = 1.0f - ay;
    const float Im = by * (bx * I00 + ax * I10) + ay * (bx * I01 + ax * I11);
    const float gx = by * (I10 - I00) + ay * (I11 - I01);
    const float gy = bx * (I01 - I00) + ax * (I11 - I10);
    const float e = pa.frame_int[i] - Im;
    if (!(std::isfinite(e) && fabsf(e) <= pa.max_diff)) return;
    float h[3], gw[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) h[j] = (gx * (P[j] - x * P[12 + j]) + gy * (P[4 + j] - y * P[12 + j])) / u3;
#pragma unroll
    for (int r = 0; r < 3; ++r) gw[r] = (Mw[r] * h[0] + Mw[4 + r] * h[1]) + Mw[8 + r] * h[2];
    const float lam = pa.weight;
    const float row[6] = {lam * (p[1] * gw[2] - p[2] * gw[1]), lam * (p[2] * gw[0] - p[0] * gw[2]),
                          lam * (p[0] * gw[1] - p[1] * gw[0]), lam * gw[0], lam * gw[1], lam * gw[2]};
    const float b = lam * e;
    if (!(std::isfinite(row[0]) && std::isfinite(row[1]) && std::isfinite(row[2]) && std::isfinite(row[3]) &&
          std::isfinite(row[4]) && std::isfinite(row[5]) && std::isfinite(b)))
        return;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const float wa = w * row[r];
#pragma unroll
        for (int s = r; s < 6; ++s) acc[k++] += (double)(wa * row[s]);
        acc[21 + r] += (double)(wa * b);
    }
    acc[TRKP_WEE] += (double)((w * e) * e);
    acc[TRKP_W] += (double)w;
    acc[TRKP_COUNT] += 1.0;
}

// The outputs of a triple for which no iteration has run, and its state
SMX_FN void trkp_begin(const TrackPhotoArgs &pa, int f) {
    trk_begin(pa.g, f, TRKP_TERMS);
    if (pa.pinfo) pa.pinfo[2 * f] = pa.pinfo[2 * f + 1] = 0;
    if (pa.prms) pa.prms[f] = __builtin_nanf("");
}

// The end of an iteration of triple f, from its TRKP_SLOTS sums
SMX_FN void trkp_finish(const TrackPhotoArgs &pa, int f, const double *S) {
    const int count = (int)S[TRKP_COUNT];
    if (pa.pinfo) {
        pa.pinfo[2 * f] = count;
        pa.pinfo[2 * f + 1] = (int)S[29] - count;
    }
    if (pa.prms) pa.prms[f] = sqrtf((float)(S[TRKP_WEE] / S[TRKP_W]));
    if (pa.g.sums)
        for (int k = 0; k < 3; ++k) pa.g.sums[(size_t)f * TRKP_TERMS + TRK_TERMS + k] = S[TRKP_WEE + k];
    trk_finish(pa.g, f, S, TRKP_TERMS);
}

}  // namespace smx
