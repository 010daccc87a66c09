// k_track_photo_rule.h -- the rule of smx_track_camera_photometric (include/stereo_mi355x.h) as plain C++ over the
// kernels' arguments: a pixel's geometric terms by k_track_rule.h's trk_pixel as it is, then its photometric terms, and
// the begin and the end of an iteration around trk_begin and trk_finish.  Compiled for the device by k_track_photo.h and
// for the host by tests/track_photo_rule_harness.cpp, which runs whole schedules on the CPU.
//
// trkp_pixel, trkp_begin and trkp_finish are written over the term's record PA, which holds the common record g, weight,
// pinfo and prms, and for which two functions say what the term reads and how it weighs it:
//   trkp_sample(pa, f, i, px, py, x, y, e, gx, gy)   the residual e of frame pixel (px, py) (index i) against the model
//                                                    plane at (x, y) and the plane's gradient there, per model pixel;
//                                                    false if the pixel has no photometric term
//   trkp_robust(pa, w, e)                            the weight of the term: w times what the residual's size earns
// This header's are the joint entry's: the full-resolution planes, and w itself.  k_track_pyramid_rule.h's read a level
// of two pyramids and weigh by Huber's rule.
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

// The bilinear interpolant of the taps I00 (x0, y0), I10 (x0 + 1, y0), I01, I11 at (x, y), and its exact gradient
SMX_FN void trkp_bilinear(float I00, float I10, float I01, float I11, float x, float x0, float y, float y0, float &Im,
                          float &gx, float &gy) {
    const float ax = x - x0, ay = y - y0, bx = 1.0f - ax, by = 1.0f - ay;
    Im = by * (bx * I00 + ax * I10) + ay * (bx * I01 + ax * I11);
    gx = by * (I10 - I00) + ay * (I11 - I01);
    gy = bx * (I01 - I00) + ax * (I11 - I10);
}

// The joint entry's sample: the four taps of the model plane around (x, y), each with a surface, against the frame's
// pixel
SMX_FN bool trkp_sample(const TrackPhotoArgs &pa, int f, size_t i, int, int, float x, float y, float &e, float &gx,
                        float &gy) {
    const TrackArgs &a = pa.g;
    const float x0 = floorf(x), y0 = floorf(y);
    if (!(x0 >= 0.0f && x0 <= (float)(a.Wm - 2) && y0 >= 0.0f && y0 <= (float)(a.Hm - 2))) return false;   // NaN fails
    const size_t plane = (size_t)a.Hm * a.Wm;
    const size_t m = (size_t)f * plane + (size_t)(int)y0 * a.Wm + (size_t)(int)x0;
    const float z00 = a.depth[m], z10 = a.depth[m + 1], z01 = a.depth[m + a.Wm], z11 = a.depth[m + a.Wm + 1];
    if (!(std::isfinite(z00) && z00 > 0.0f && std::isfinite(z10) && z10 > 0.0f && std::isfinite(z01) && z01 > 0.0f &&
          std::isfinite(z11) && z11 > 0.0f))
        return false;
    const float I00 = pa.model_int[m], I10 = pa.model_int[m + 1], I01 = pa.model_int[m + a.Wm];
    const float I11 = pa.model_int[m + a.Wm + 1];
    if (!(std::isfinite(I00) && std::isfinite(I10) && std::isfinite(I01) && std::isfinite(I11))) return false;
    float Im;
    trkp_bilinear(I00, I10, I01, I11, x, x0, y, y0, Im, gx, gy);
    e = pa.frame_int[i] - Im;
    return std::isfinite(e) && fabsf(e) <= pa.max_diff;
}

SMX_FN float trkp_robust(const TrackPhotoArgs &, float w, float) { return w; }

// Adds the terms of pixel (px, py) of frame f at the pose T to acc: the geometric ones, and after them, if the pixel was
// a geometric inlier, the photometric ones.  The values the two parts share (p, u, w) are evaluated again, by calls of
// the functions of k_camera.h that trk_pixel calls, on the same operands (keeping them across trk_pixel instead would be
// this kernel's register decision).
template <class PA> SMX_FN void trkp_pixel(const PA &pa, const float *T, int f, int px, int py, double acc[TRKP_SLOTS]) {
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
    float e, gx, gy;
    if (!trkp_sample(pa, f, i, px, py, x, y, e, gx, gy)) return;
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
    const float wp = trkp_robust(pa, w, e);
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const float wa = wp * row[r];
#pragma unroll
        for (int s = r; s < 6; ++s) acc[k++] += (double)(wa * row[s]);
        acc[21 + r] += (double)(wa * b);
    }
    acc[TRKP_WEE] += (double)((wp * e) * e);
    acc[TRKP_W] += (double)wp;
    acc[TRKP_COUNT] += 1.0;
}

// The outputs of a triple for which no iteration has run, and its state
template <class PA> SMX_FN void trkp_begin(const PA &pa, int f) {
    trk_begin(pa.g, f, TRKP_TERMS);
    if (pa.pinfo) pa.pinfo[2 * f] = pa.pinfo[2 * f + 1] = 0;
    if (pa.prms) pa.prms[f] = __builtin_nanf("");
}

// The end of an iteration of triple f, from its TRKP_SLOTS sums
template <class PA> SMX_FN void trkp_finish(const PA &pa, int f, const double *S) {
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

// The joint rule as k_track_body.h takes a rule, over the term's record PA and the shape of its combine (k_track_photo.h)
template <class PA, int COMBINE_CHUNKS, int COMBINE_STACK> struct TrackJointRule {
    using Args = PA;
    static constexpr int SLOTS = TRKP_SLOTS, BUTTERFLY = TRKP_SLOTS, CHUNKS = COMBINE_CHUNKS, STACK = COMBINE_STACK;
    static SMX_FN TrackArgs &common(PA &a) { return a.g; }
    static SMX_FN const TrackArgs &common(const PA &a) { return a.g; }
    static SMX_FN void pixel(const PA &a, const float *T, int f, int px, int py, double *acc) {
        trkp_pixel(a, T, f, px, py, acc);
    }
    static SMX_FN void begin(const PA &a, int f) { trkp_begin(a, f); }
    static SMX_FN void finish(const PA &a, int f, const double *S) { trkp_finish(a, f, S); }
};

}  // namespace smx
