// k_track_pyramid_rule.h -- the rules of smx_intensity_pyramid and smx_track_camera_pyramid (include/stereo_mi355x.h) as
// plain C++ (the places of a pyramid's levels are smx_workspace.h's): the five-tap reduce, and what the joint rule of
// k_track_photo_rule.h reads and how it weighs it when its planes are a level of two pyramids.  Everything else of the
// tracking rule -- the geometric terms, the projection, the row of the system, the sums, the begin and the end of an
// iteration -- is k_track_photo_rule.h's, instantiated for this header's record.  Compiled for the device by k_pyramid.h
// and k_track_pyramid.h and for the host by tests/track_pyramid_rule_harness.cpp.
#pragma once
#include "k_track_photo_rule.h"

namespace smx {

// Burt and Adelson's five taps (1 4 6 4 1) / 16 over a[-2] .. a[2], one float32 operation per step
SMX_FN float pyr_taps(float m2, float m1, float c, float p1, float p2) {
    return (((m2 + p2) + 4.0f * (m1 + p1)) + 6.0f * c) * 0.0625f;
}

SMX_FN int pyr_clamp(int i, int size) { return i < 0 ? 0 : i > size - 1 ? size - 1 : i; }

// The horizontal pass at row r (in the plane), output column x, of the plane a [H][W]
SMX_FN float pyr_reduce_row(const float *a, int W, int r, int x) {
    const float *row = a + (size_t)r * W;
    return pyr_taps(row[pyr_clamp(2 * x - 2, W)], row[pyr_clamp(2 * x - 1, W)], row[pyr_clamp(2 * x, W)],
                    row[pyr_clamp(2 * x + 1, W)], row[pyr_clamp(2 * x + 2, W)]);
}

// Level pixel (x, y) of the next level from the plane a [H][W]: the rule, tap by tap.  k_pyramid.h computes the same
// values from a tile in LDS.
SMX_FN float pyr_reduce_pixel(const float *a, int H, int W, int x, int y) {
    return pyr_taps(pyr_reduce_row(a, W, pyr_clamp(2 * y - 2, H), x), pyr_reduce_row(a, W, pyr_clamp(2 * y - 1, H), x),
                    pyr_reduce_row(a, W, pyr_clamp(2 * y, H), x), pyr_reduce_row(a, W, pyr_clamp(2 * y + 1, H), x),
                    pyr_reduce_row(a, W, pyr_clamp(2 * y + 2, H), x));
}

struct TrackPyramidArgs {
    TrackArgs g;                                                     // sums: [n][TRKP_TERMS]; the partials hold TRKP_SLOTS
    // this schedule pair's level of the two pyramids (k_track_body.h: track_launch's per_pair)
    const float *__restrict__ frame_lvl, *__restrict__ model_lvl;    // [n][Hl][Wl], [n][Hml][Wml]
    int shift, Hl, Wl, Hml, Wml;                                     // the level, and its dimensions in both pyramids
    float inv;                                                       // 2^-level
    float weight, max_diff, huber;                                   // lambda, max_intensity_difference, huber_delta
    int *pinfo;                                                      // [n][2], may be NULL
    float *prms;                                                     // [n], may be NULL
};

// The sample of a level: the model pyramid's four taps around (x, y) / 2^level, finite only where every pixel beneath
// them had a surface, against the frame pyramid's pixel above (px, py); the gradient comes back per level-0 pixel
SMX_FN bool trkp_sample(const TrackPyramidArgs &pa, int f, size_t, int px, int py, float x, float y, float &e, float &gx,
                        float &gy) {
    const float xl = x * pa.inv, yl = y * pa.inv;
    const float x0 = floorf(xl), y0 = floorf(yl);
    if (!(x0 >= 0.0f && x0 <= (float)(pa.Wml - 2) && y0 >= 0.0f && y0 <= (float)(pa.Hml - 2))) return false;   // NaN fails
    const size_t m = ((size_t)f * pa.Hml + (size_t)(int)y0) * pa.Wml + (size_t)(int)x0;
    const float I00 = pa.model_lvl[m], I10 = pa.model_lvl[m + 1], I01 = pa.model_lvl[m + pa.Wml];
    const float I11 = pa.model_lvl[m + pa.Wml + 1];
    if (!(std::isfinite(I00) && std::isfinite(I10) && std::isfinite(I01) && std::isfinite(I11))) return false;
    float Im, gxl, gyl;
    trkp_bilinear(I00, I10, I01, I11, xl, x0, yl, y0, Im, gxl, gyl);
    gx = gxl * pa.inv, gy = gyl * pa.inv;
    e = pa.frame_lvl[((size_t)f * pa.Hl + (py >> pa.shift)) * pa.Wl + (px >> pa.shift)] - Im;
    return std::isfinite(e) && fabsf(e) <= pa.max_diff;
}

// Huber's weight: 1 up to huber_delta, huber_delta / |e| beyond it
SMX_FN float trkp_robust(const TrackPyramidArgs &pa, float w, float e) {
    const float ae = fabsf(e);
    const float wh = ae <= pa.huber ? 1.0f : pa.huber / ae;
    return w * wh;
}

}  // namespace smx
