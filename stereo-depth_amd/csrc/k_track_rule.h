// k_track_rule.h -- the rule of smx_track_camera (include/stereo_mi355x.h) as plain C++ over the kernels' arguments:
// the thirty terms of one pixel, and the solve and pose update of one iteration.  Compiled for the device by k_track.h
// and for the host by tests/track_rule_harness.cpp, which runs whole schedules on the CPU.
#pragma once
#include <cmath>

#include "k_camera.h"
#include "smx_workspace.h"

namespace smx {

// What a triple carries from launch to launch (workspace, one per triple; 32 words)
struct TrackState {
    float pose[12];                  // T: the current camera-to-world estimate
    float pose0[12];                 // pose_in's bits, for a LOST triple
    int done, lost, iterations, pad[5];
};

struct TrackArgs {
    int n, H, W, Hm, Wm;
    const float *__restrict__ disp, *__restrict__ conf;              // [n][H][W]; conf NULL: every accepted pixel weighs 1
    const float *__restrict__ depth, *__restrict__ normals;          // [n][Hm][Wm], [n][3][Hm][Wm]
    const float *__restrict__ c2w, *__restrict__ w2c;                // [n][3][4] each: the model views' poses
    float q[16], qm[16], pm[16];
    float min_conf, zmin, zmax, invalid, maxd2;                      // maxd2 = max_distance * max_distance
    int stride, ws, hs, tx, tiles, groups;                           // this iteration's TrackGrid
    int min_inliers;
    double min_pivot;
    float rot_eps2, trans_eps2;
    const float *pose_in;                                            // [n][3][4]
    float *pose_out, *rms;                                           // rms and the outputs below may be NULL
    int *info;                                                       // [n][4]
    double *sums;                                                    // [n][the rule's terms]
    TrackState *state;                                               // workspace [n]
    double *partial;                                                 // workspace [n][groups of stride 1][the rule's slots]
    size_t partial_stride;                                           // doubles per triple
};

// Adds the thirty terms of pixel (px, py) of frame f at the pose T to acc, and 1 to acc[TRK_TERMS] if the pixel is
// accepted.  A skipped pixel adds nothing: acc starts at +0.0 and a sum of these terms is never -0.0, so leaving the
// addition of +0.0 out changes no bit.
SMX_FN void trk_pixel(const TrackArgs &a, const float *T, int f, int px, int py, double acc[TRK_SLOTS]) {
    const size_t i = ((size_t)f * a.H + py) * a.W + px;
    const float d = a.disp[i];
    if (!(std::isfinite(d) && d != a.invalid)) return;
    const float u = (float)px, v = (float)py;
    const float *q = a.q;
    const float ww = affine_row(q, 3, u, v, d);
    if (!(ww > 0.0f)) return;
    const float Z = affine_row(q, 2, u, v, d) / ww;
    if (!(std::isfinite(Z) && Z >= a.zmin && Z <= a.zmax)) return;
    float w = 1.0f;
    if (a.conf) {
        w = a.conf[i];
        if (!(w >= a.min_conf && w > 0.0f)) return;                   // a NaN confidence excludes the pixel
    }
    const float X = affine_row(q, 0, u, v, d) / ww, Y = affine_row(q, 1, u, v, d) / ww;
    if (!(std::isfinite(X) && std::isfinite(Y))) return;
    acc[TRK_TERMS] += 1.0;
    const float p[3] = {affine_row(T, 0, X, Y, Z), affine_row(T, 1, X, Y, Z), affine_row(T, 2, X, Y, Z)};
    const float *Mw = a.w2c + (size_t)f * 12, *Mc = a.c2w + (size_t)f * 12;
    const float c[3] = {affine_row(Mw, 0, p[0], p[1], p[2]), affine_row(Mw, 1, p[0], p[1], p[2]),
                        affine_row(Mw, 2, p[0], p[1], p[2])};
    if (!(c[2] > 0.0f)) return;
    const float *P = a.pm;
    const float p3 = affine_row(P, 3, c[0], c[1], c[2]);
    if (!(p3 > 0.0f)) return;
    const float fu = nearest_pixel(affine_row(P, 0, c[0], c[1], c[2]), p3);
    const float fv = nearest_pixel(affine_row(P, 1, c[0], c[1], c[2]), p3);
    if (!(fu >= 0.0f && fu <= (float)(a.Wm - 1) && fv >= 0.0f && fv <= (float)(a.Hm - 1))) return;   // NaN fails
    const size_t plane = (size_t)a.Hm * a.Wm;
    const size_t m = (size_t)(int)fv * a.Wm + (size_t)(int)fu;
    const float lam = a.depth[(size_t)f * plane + m];
    if (!(std::isfinite(lam) && lam > 0.0f)) return;
    const float *nr = a.normals + (size_t)f * 3 * plane + m;
    const float n0 = nr[0], n1 = nr[plane], n2 = nr[2 * plane];
    if (n0 == 0.0f && n1 == 0.0f && n2 == 0.0f) return;
    const float *qm = a.qm;
    const float xp = pixel_ray_row(qm, 0, fu, fv), yp = pixel_ray_row(qm, 1, fu, fv), zp = pixel_ray_row(qm, 2, fu, fv);
    const float rx = xp / zp, ry = yp / zp;
    float dl[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float dw = rotation_row(Mc, r, rx, ry);
        dl[r] = (Mc[4 * r + 3] + dw * lam) - p[r];
    }
    if (!((dl[0] * dl[0] + dl[1] * dl[1]) + dl[2] * dl[2] <= a.maxd2)) return;                        // NaN fails
    const float b = (n0 * dl[0] + n1 * dl[1]) + n2 * dl[2];
    const float row[6] = {p[1] * n2 - p[2] * n1, p[2] * n0 - p[0] * n2, p[0] * n1 - p[1] * n0, n0, n1, n2};
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
        const float wa = w * row[r];
#pragma unroll
        for (int s = r; s < 6; ++s) acc[k++] += (double)(wa * row[s]);
        acc[21 + r] += (double)(wa * b);
    }
    acc[27] += (double)((w * b) * b);
    acc[28] += (double)w;
    acc[29] += 1.0;
}

// x of A x = g by LDL^T without pivoting, in the header's order; false when a pivot is not finite or <= min_pivot or a
// component of x is not finite
SMX_FN bool trk_solve(const double *S, double min_pivot, double x[6]) {
    double A[6][6], L[6][6], d[6], v[6], y[6];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) A[i][j] = A[j][i] = S[k++];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
#pragma unroll
        for (int c = 0; c < j; ++c) v[c] = L[j][c] * d[c];
        double s = A[j][j];
#pragma unroll
        for (int c = 0; c < j; ++c) s = s - L[j][c] * v[c];
        if (!(std::isfinite(s) && s > min_pivot)) return false;
        d[j] = s;
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double t = A[i][j];
#pragma unroll
            for (int c = 0; c < j; ++c) t = t - L[i][c] * v[c];
            L[i][j] = t / d[j];
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = S[21 + i];
#pragma unroll
        for (int c = 0; c < i; ++c) s = s - L[i][c] * y[c];
        y[i] = s;
    }
    bool finite = true;
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        double s = y[i] / d[i];
#pragma unroll
        for (int c = i + 1; c < 6; ++c) s = s - L[c][i] * x[c];
        x[i] = s;
        finite = finite && std::isfinite(s);
    }
    return finite;
}

// T <- (C T, C t + tau) with C the Cayley map of omega; returns true iff the step is within the tolerances
SMX_FN bool trk_update(float *T, const double x[6], float rot_eps2, float trans_eps2) {
    const float om[3] = {(float)x[0], (float)x[1], (float)x[2]}, tau[3] = {(float)x[3], (float)x[4], (float)x[5]};
    const float a0 = om[0] * 0.5f, a1 = om[1] * 0.5f, a2 = om[2] * 0.5f;
    const float aa = (a0 * a0 + a1 * a1) + a2 * a2;
    const float den = 1.0f + aa, k = 1.0f - aa;
    const float t0 = 2.0f * a0, t1 = 2.0f * a1, t2 = 2.0f * a2;
    const float C[3][3] = {{(k + t0 * a0) / den, (t0 * a1 - t2) / den, (t0 * a2 + t1) / den},
                           {(t1 * a0 + t2) / den, (k + t1 * a1) / den, (t1 * a2 - t0) / den},
                           {(t2 * a0 - t1) / den, (t2 * a1 + t0) / den, (k + t2 * a2) / den}};
    float out[12];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) out[4 * r + c] = (C[r][0] * T[c] + C[r][1] * T[4 + c]) + C[r][2] * T[8 + c];
        out[4 * r + 3] = ((C[r][0] * T[3] + C[r][1] * T[7]) + C[r][2] * T[11]) + tau[r];
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) T[i] = out[i];
    return (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2] <= rot_eps2 &&
           (tau[0] * tau[0] + tau[1] * tau[1]) + tau[2] * tau[2] <= trans_eps2;
}

// The outputs of a triple for which no iteration has run (the first launch of a call writes them, so a schedule of zero
// iterations is the identity), and its state.  terms: the sums per triple of the rule that is tracked, this one's or more.
SMX_FN void trk_begin(const TrackArgs &a, int f, int terms = TRK_TERMS) {
    TrackState &st = a.state[f];
    float in[12];
    for (int i = 0; i < 12; ++i) in[i] = a.pose_in[(size_t)f * 12 + i];   // read whole before pose_out, which may be it
    for (int i = 0; i < 12; ++i) st.pose[i] = st.pose0[i] = a.pose_out[(size_t)f * 12 + i] = in[i];
    st.done = st.lost = st.iterations = 0;
    if (a.info) a.info[4 * f] = a.info[4 * f + 1] = a.info[4 * f + 2] = a.info[4 * f + 3] = 0;
    if (a.rms) a.rms[f] = __builtin_nanf("");
    if (a.sums)
        for (int k = 0; k < terms; ++k) a.sums[(size_t)f * terms + k] = 0.0;
}

// The end of an iteration of triple f, from its sums: the outputs (the first TRK_TERMS of the triple's `terms` sums), the
// new pose, the stop flags
SMX_FN void trk_finish(const TrackArgs &a, int f, const double *S, int terms = TRK_TERMS) {
    TrackState &st = a.state[f];
    const int inliers = (int)S[29];
    st.iterations += 1;
    if (a.info) {
        a.info[4 * f + 1] = st.iterations;
        a.info[4 * f + 2] = inliers;
        a.info[4 * f + 3] = (int)S[TRK_TERMS];
    }
    if (a.rms) a.rms[f] = sqrtf((float)(S[27] / S[28]));
    if (a.sums)
        for (int k = 0; k < TRK_TERMS; ++k) a.sums[(size_t)f * terms + k] = S[k];
    double x[6];
    const bool ok = inliers >= a.min_inliers && trk_solve(S, a.min_pivot, x);
    float *out = a.pose_out + (size_t)f * 12;
    if (!ok) {
        st.done = st.lost = 1;
        if (a.info) a.info[4 * f] = 1;
        for (int i = 0; i < 12; ++i) out[i] = st.pose0[i];
        return;
    }
    float T[12];
    for (int i = 0; i < 12; ++i) T[i] = st.pose[i];
    if (trk_update(T, x, a.rot_eps2, a.trans_eps2)) st.done = 1;
    for (int i = 0; i < 12; ++i) st.pose[i] = out[i] = T[i];
}

}  // namespace smx
