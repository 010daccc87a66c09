// track_pyramid_rule_harness.cpp -- smx_intensity_pyramid and smx_track_camera_pyramid on the CPU: the library's own reduce
// rule, per-pixel terms, solve and pose update (stereo-depth_amd/csrc/k_track_pyramid_rule.h over k_track_photo_rule.h
// and k_track_rule.h, the code the kernels run) over whole schedules, with the pyramids built pixel by pixel from
// pyr_reduce_pixel and the sums taken in the header's order by plain loops: tile columns top to bottom, then an
// adjacent-pairs tree over the 64 columns, then one over the tiles.  tests/test_track_pyramid_rule_cpu.py compares every
// output bit for bit with the NumPy twin.
//
//   track_pyramid_rule_harness IN OUT
// IN:  int32 n H W Hm Wm has_conf pairs min_inliers levels | int32 schedule[8][2] | int32 schedule_levels[8] |
//      f32 min_conf zmin zmax invalid max_distance min_pivot rot_eps trans_eps weight max_difference huber_delta |
//      f32 Q[16] Qm[16] Pm[16] | f32 c2w[n][12] w2c[n][12] pose_in[n][12] | f32 disp[n H W] | f32 conf[n H W] (with
//      has_conf) | f32 depth[n Hm Wm] | f32 normals[n 3 Hm Wm] | f32 frame_intensity[n H W] | f32 model_intensity[n Hm Wm]
// OUT: f32 pose[n][12] | int32 info[n][4] | f32 rms[n] | f64 sums[n][33] | int32 pinfo[n][2] | f32 prms[n] |
//      f32 frame pyramid | f32 model pyramid (masked by depth), in smx_intensity_pyramid's layout
// Prints "track-pyramid-rule triples N iterations I": the iterations that ran, over all triples.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "k_track_pyramid_rule.h"

constexpr int SLOTS = smx::TRKP_SLOTS;

template <class T> static void get(FILE *f, T *p, size_t count) {
    if (fread(p, sizeof(T), count, f) != count) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

// adjacent pairs first, padded with +0.0 to a power of two; v: [count][SLOTS]
static void pairs_tree(std::vector<double> &v, size_t count, double out[SLOTS]) {
    size_t p = 1;
    while (p < count) p *= 2;
    v.resize(p * SLOTS, 0.0);
    for (; p > 1; p /= 2)
        for (size_t i = 0; i < p / 2; ++i)
            for (int k = 0; k < SLOTS; ++k) v[i * SLOTS + k] = v[2 * i * SLOTS + k] + v[(2 * i + 1) * SLOTS + k];
    for (int k = 0; k < SLOTS; ++k) out[k] = v[k];
}

// smx_intensity_pyramid by its rule
static std::vector<float> pyramid(int n, int H, int W, int levels, const std::vector<float> &plane, const float *mask) {
    std::vector<float> out(smx::pyramid_level(n, H, W, levels).offset);
    for (size_t i = 0; i < plane.size(); ++i)
        out[i] = !mask || (std::isfinite(mask[i]) && mask[i] > 0.0f) ? plane[i] : __builtin_nanf("");
    for (int l = 1; l < levels; ++l) {
        const smx::PyramidLevel from = smx::pyramid_level(n, H, W, l - 1), to = smx::pyramid_level(n, H, W, l);
        for (int f = 0; f < n; ++f)
            for (int y = 0; y < to.H; ++y)
                for (int x = 0; x < to.W; ++x)
                    out[to.offset + ((size_t)f * to.H + y) * to.W + x] =
                        smx::pyr_reduce_pixel(out.data() + from.offset + (size_t)f * from.H * from.W, from.H, from.W, x, y);
    }
    return out;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[9], schedule[16], slevels[8];
    float pr[11];
    get(f, hd, 9);
    get(f, schedule, 16);
    get(f, slevels, 8);
    get(f, pr, 11);
    smx::TrackPyramidArgs pa;
    memset(&pa, 0, sizeof(pa));
    smx::TrackArgs &a = pa.g;
    a.n = hd[0], a.H = hd[1], a.W = hd[2], a.Hm = hd[3], a.Wm = hd[4];
    const bool has_conf = hd[5] != 0;
    const int pairs = hd[6], levels = hd[8];
    a.min_inliers = hd[7];
    a.min_conf = pr[0], a.zmin = pr[1], a.zmax = pr[2], a.invalid = pr[3], a.maxd2 = pr[4] * pr[4];
    a.min_pivot = (double)pr[5], a.rot_eps2 = pr[6] * pr[6], a.trans_eps2 = pr[7] * pr[7];
    pa.weight = pr[8], pa.max_diff = pr[9], pa.huber = pr[10];
    get(f, a.q, 16);
    get(f, a.qm, 16);
    get(f, a.pm, 16);
    const size_t n = (size_t)a.n, px = n * a.H * a.W, mpx = n * a.Hm * a.Wm;
    std::vector<float> c2w(n * 12), w2c(n * 12), pose_in(n * 12), disp(px), conf(has_conf ? px : 0), depth(mpx);
    std::vector<float> normals(3 * mpx), fint(px), mint(mpx);
    get(f, c2w.data(), c2w.size());
    get(f, w2c.data(), w2c.size());
    get(f, pose_in.data(), pose_in.size());
    get(f, disp.data(), px);
    if (has_conf) get(f, conf.data(), px);
    get(f, depth.data(), mpx);
    get(f, normals.data(), 3 * mpx);
    get(f, fint.data(), px);
    get(f, mint.data(), mpx);
    fclose(f);
    const std::vector<float> fpyr = pyramid(a.n, a.H, a.W, levels, fint, nullptr);
    const std::vector<float> mpyr = pyramid(a.n, a.Hm, a.Wm, levels, mint, depth.data());
    std::vector<float> pose_out(n * 12), rms(n), prms(n);
    std::vector<int> info(n * 4), pinfo(n * 2);
    std::vector<double> sums(n * smx::TRKP_TERMS);
    std::vector<smx::TrackState> state(n);
    a.disp = disp.data(), a.conf = has_conf ? conf.data() : nullptr, a.depth = depth.data(), a.normals = normals.data();
    a.c2w = c2w.data(), a.w2c = w2c.data(), a.pose_in = pose_in.data();
    a.pose_out = pose_out.data(), a.rms = rms.data(), a.info = info.data(), a.sums = sums.data(), a.state = state.data();
    pa.pinfo = pinfo.data(), pa.prms = prms.data();
    long ran = 0;
    for (int t = 0; t < a.n; ++t) smx::trkp_begin(pa, t);
    for (int p = 0; p < pairs; ++p) {
        const smx::TrackGrid g = smx::track_grid(a.H, a.W, schedule[2 * p]);
        a.stride = schedule[2 * p];
        const smx::PyramidLevel fl = smx::pyramid_level(a.n, a.H, a.W, slevels[p]);
        const smx::PyramidLevel ml = smx::pyramid_level(a.n, a.Hm, a.Wm, slevels[p]);
        pa.frame_lvl = fpyr.data() + fl.offset, pa.model_lvl = mpyr.data() + ml.offset;
        pa.shift = slevels[p], pa.Hl = fl.H, pa.Wl = fl.W, pa.Hml = ml.H, pa.Wml = ml.W;
        pa.inv = 1.0f / (float)(1 << slevels[p]);
        for (int it = 0; it < schedule[2 * p + 1]; ++it)
            for (int t = 0; t < a.n; ++t) {
                if (state[t].done) continue;
                std::vector<double> tiles((size_t)g.tiles * SLOTS, 0.0);
                for (int ty = 0; ty < g.ty; ++ty)
                    for (int tx = 0; tx < g.tx; ++tx) {
                        std::vector<double> cols((size_t)smx::TRK_COLS * SLOTS, 0.0);
                        for (int c = 0; c < smx::TRK_COLS; ++c)
                            for (int r = 0; r < smx::TRK_ROWS; ++r) {
                                const int sx = tx * smx::TRK_COLS + c, sy = ty * smx::TRK_ROWS + r;
                                if (sx < g.ws && sy < g.hs)
                                    smx::trkp_pixel(pa, state[t].pose, t, sx * a.stride, sy * a.stride,
                                                    &cols[(size_t)c * SLOTS]);
                            }
                        pairs_tree(cols, smx::TRK_COLS, &tiles[((size_t)ty * g.tx + tx) * SLOTS]);
                    }
                double S[SLOTS];
                pairs_tree(tiles, (size_t)g.tiles, S);
                smx::trkp_finish(pa, t, S);
                ++ran;
            }
    }
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(pose_out.data(), 4, pose_out.size(), o);
    fwrite(info.data(), 4, info.size(), o);
    fwrite(rms.data(), 4, rms.size(), o);
    fwrite(sums.data(), 8, sums.size(), o);
    fwrite(pinfo.data(), 4, pinfo.size(), o);
    fwrite(prms.data(), 4, prms.size(), o);
    fwrite(fpyr.data(), 4, fpyr.size(), o);
    fwrite(mpyr.data(), 4, mpyr.size(), o);
    fclose(o);
    printf("track-pyramid-rule triples %d iterations %ld\n", a.n, ran);
    return 0;
}
