/*
 * driver.cc -- one C entry that runs the reference's own stereo_matching class on the host, step by step, and copies
 * out its buffers after the steps that tests/golden/make_golden.py names (our own code; test infrastructure only).
 *
 * The steps of the class are private, and which arguments it hands to each kernel wrapper (min_disparity / K in
 * integer division among them) is exactly what is to be pinned, so the class is used as it stands: its header is
 * read here with `private` spelled `public`.  Its translation unit is compiled untouched; the layout is the same.
 */
#include <cstring>

#include "ref_host.h"

#define private public
#include "depth/stereo_matching.hh"
#undef private

namespace {

void copy_out(const torch::Tensor &t, float *dst) {
    if (dst) std::memcpy(dst, t.data_ptr<float>(), sizeof(float) * static_cast<size_t>(t.numel()));
}

}  // namespace

/* cfg = the eleven fields in the order of stereo_matching_configuration.hh: [H, W, K, min_disparity, max_disparity,
 * ncc_patch_radius, sad_patch_radius, threshold, small_mbm_radius, mid_mbm_radius, large_mbm_radius].  The caller keeps
 * small, mid <= large: the aggregation kernel's tile is sized by the large radius and the reference indexes past it
 * otherwise.  left/right float32 [3,H,W] (rgb != 0) or [H,W]; every sink may be NULL.  Sizes: out, gray_left [H,W];
 * down_left, wta, refined [h,w]; agg [h,w,Dd] (h, w, Dd as the reference's device_buffer derives them).  Returns 0. */
extern "C" int ref_host_run(const int32_t *cfg, const float *left, const float *right, int rgb, float poison, int reverse,
                            float *out, float *gray_left, float *down_left, float *wta, float *refined, float *agg) {
    refhost::set_poison(poison);
    refhost::set_reverse(reverse != 0);

    stereo_matching_configuration c;
    c.height = static_cast<uint32_t>(cfg[0]);
    c.width = static_cast<uint32_t>(cfg[1]);
    c.downscale_factor = static_cast<uint32_t>(cfg[2]);
    c.min_disparity = cfg[3];
    c.max_disparity = cfg[4];
    c.ncc_patch_radius = static_cast<uint32_t>(cfg[5]);
    c.sad_patch_radius = static_cast<uint32_t>(cfg[6]);
    c.threshold = static_cast<uint32_t>(cfg[7]);
    c.small_mbm_radius = cfg[8];
    c.mid_mbm_radius = cfg[9];
    c.large_mbm_radius = cfg[10];
    stereo_matching sm(c);

    const size_t plane = static_cast<size_t>(cfg[0]) * static_cast<size_t>(cfg[1]);
    if (rgb) {
        torch::Tensor l = torch::empty({3, cfg[0], cfg[1]}), r = torch::empty({3, cfg[0], cfg[1]});
        std::memcpy(l.data_ptr<float>(), left, 3 * plane * sizeof(float));
        std::memcpy(r.data_ptr<float>(), right, 3 * plane * sizeof(float));
        sm.grayscale(l, r);
    } else {
        std::memcpy(sm.m_buffer.left_grayscaled.data_ptr<float>(), left, plane * sizeof(float));
        std::memcpy(sm.m_buffer.right_grayscaled.data_ptr<float>(), right, plane * sizeof(float));
    }
    copy_out(sm.m_buffer.left_grayscaled, gray_left);
    sm.downscale();
    copy_out(sm.m_buffer.left_downscaled, down_left);
    sm.ncc_matching_cost_volume_construction();
    sm.multi_block_matching_cost_aggregation();
    copy_out(sm.m_buffer.aggregated_cost_volume, agg);
    sm.wta_disparity_selection();
    copy_out(sm.m_buffer.downscaled_disparity, wta);
    sm.secondary_matching();
    copy_out(sm.m_buffer.downscaled_disparity, refined);
    sm.upscale_disparity_vertical_fill();
    sm.horizontal_disparity_fill();
    copy_out(sm.m_buffer.output_disparity, out);
    return 0;
}

/* [h, w, Dd] of a configuration, from the reference's own buffer constructor. */
extern "C" void ref_host_dims(const int32_t *cfg, int32_t *hwd) {
    device_buffer b(static_cast<uint32_t>(cfg[0]), static_cast<uint32_t>(cfg[1]), cfg[3], cfg[4], static_cast<uint32_t>(cfg[2]));
    for (int i = 0; i < 3; i++) hwd[i] = static_cast<int32_t>(b.aggregated_cost_volume.size(i));
}
