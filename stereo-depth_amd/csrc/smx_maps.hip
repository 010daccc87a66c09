// smx_maps.hip -- the engine-free entries of the C ABI of include/stereo_mi355x.h: operations on maps and frames the
// caller already has, checked here and enqueued on the caller's stream through the launchers of smx_launch.h.
#include <cstdio>
#include <initializer_list>
#include <type_traits>

#include "smx_launch.h"
#include "smx_status.h"
#include "smx_workspace.h"

using namespace smx;

static bool map_dims_ok(int n, int H, int W) { return n >= 1 && H >= 1 && W >= 1 && H <= 32768 && W <= 32768; }

static int check_map_dims(const char *fn, int n, int H, int W) {
    if (map_dims_ok(n, H, W)) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: need n >= 1 and 1 <= H, W <= 32768 (got n %d, H %d, W %d)", fn, n, H, W);
}

static int check_caller_stream(const char *fn, void *stream) {
    return stream == SMX_STREAM_ENGINE ? fail(SMX_ERR_INVALID_ARG, "%s needs a caller stream", fn) : SMX_OK;
}

// A caller-supplied workspace must be 256-byte aligned (include/stereo_mi355x.h: conventions): the layouts inside it are
// rounded to 256 bytes and hold 8-byte values and atomics.  NULL passes: each entry has its own rule for it.
static int check_workspace_alignment(const char *fn, const void *workspace) {
    if (((uintptr_t)workspace & 255u) == 0) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: the workspace must be 256-byte aligned (got %p)", fn, workspace);
}

// The last two host checks of every entry that takes a workspace.
static int check_workspace_and_stream(const char *fn, const void *workspace, void *stream) {
    if (int rc = check_workspace_alignment(fn, workspace)) return rc;
    return check_caller_stream(fn, stream);
}

// ---- one spelling per kind of rule ---------------------------------------------------------------------------------
static int check_positive(const char *fn, const char *name, float v) {
    if (std::isfinite(v) && v > 0.0f) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: %s must be finite and > 0, got %g", fn, name, (double)v);
}

static int check_non_negative(const char *fn, const char *name, float v) {
    if (std::isfinite(v) && v >= 0.0f) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: %s must be finite and >= 0, got %g", fn, name, (double)v);
}

static int check_int_range(const char *fn, const char *name, int v, int lo, int hi) {
    if (v >= lo && v <= hi) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: %s must be in %d..%d, got %d", fn, name, lo, hi, v);
}

static int check_finite_at(const char *fn, const char *name, const float *v, int k) {
    if (std::isfinite(v[k])) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: %s[%d] = %g is not finite", fn, name, k, (double)v[k]);
}

static int check_finite_array(const char *fn, const char *name, const float *v, int count) {
    for (int k = 0; k < count; ++k)
        if (int rc = check_finite_at(fn, name, v, k)) return rc;
    return SMX_OK;
}

// `query`: the name of the entry's size query, whose value for these arguments is `need`.
static int check_workspace_bytes(const char *fn, const char *query, size_t workspace_bytes, size_t need) {
    if (workspace_bytes >= need) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: workspace_bytes %zu is below %s = %zu", fn, workspace_bytes, query, need);
}

// what: "" or "image "
static int check_dtype(const char *fn, const char *what, int dtype) {
    if (dtype == SMX_DTYPE_U8 || dtype == SMX_DTYPE_F32) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: unknown %sdtype %d", fn, what, dtype);
}

static constexpr long SMX_POINTS_MAX = 1L << 30;     // n*H*W (reprojection, TSDF integration) and every capacity

static int check_capacity(const char *fn, int capacity) {
    if (capacity >= 1 && capacity <= SMX_POINTS_MAX) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: capacity must be in 1..2^30, got %d", fn, capacity);
}

static bool points_dims_ok(int n, int H, int W) { return map_dims_ok(n, H, W) && (long)n * H * W <= SMX_POINTS_MAX; }

// After check_map_dims.
static int check_pixel_count(const char *fn, int n, int H, int W) {
    if ((long)n * H * W <= SMX_POINTS_MAX) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: n * H * W = %ld exceeds 2^30: split the batch", fn, (long)n * H * W);
}

// An operand's bytes; a NULL operand overlaps nothing.
struct Span {
    const void *p;
    size_t bytes;
};

// Each of `outs` in turn: it must overlap none of `ins` (else in_text) and, where out_text is given, none of the outs
// after it (else out_text).  The texts are the entry's own.
static int check_disjoint(const char *fn, std::initializer_list<Span> ins, std::initializer_list<Span> outs,
                          const char *in_text, const char *out_text = nullptr) {
    for (const Span *o = outs.begin(); o != outs.end(); ++o) {
        for (const Span &i : ins)
            if (ranges_overlap(o->p, o->bytes, i.p, i.bytes)) return fail(SMX_ERR_INVALID_ARG, "%s: %s", fn, in_text);
        for (const Span *q = o + 1; out_text && q != outs.end(); ++q)
            if (ranges_overlap(o->p, o->bytes, q->p, q->bytes)) return fail(SMX_ERR_INVALID_ARG, "%s: %s", fn, out_text);
    }
    return SMX_OK;
}

// The rules smx_reproject_points and smx_tsdf_integrate share, in their order; colour_out: the output that needs an
// image, colour_text: what the entry says when it has none.
static int check_reprojection_args(const char *fn, float z_min, float z_max, float min_confidence, float invalid_disparity,
                                   const void *image, int image_channels, int image_dtype, const void *colour_out,
                                   const char *colour_text) {
    if (std::isnan(z_min) || std::isnan(z_max) || z_min > z_max)
        return fail(SMX_ERR_INVALID_ARG, "%s: need z_min <= z_max, got %g, %g", fn, (double)z_min, (double)z_max);
    if (!std::isfinite(min_confidence))
        return fail(SMX_ERR_INVALID_ARG, "%s: min_confidence must be finite, got %g", fn, (double)min_confidence);
    if (int rc = check_finite_marker(invalid_disparity)) return rc;
    if (image) {
        if (image_channels != 1 && image_channels != 3)
            return fail(SMX_ERR_INVALID_ARG, "%s: image_channels must be 1 or 3 with an image, got %d", fn, image_channels);
        return check_dtype(fn, "image ", image_dtype);
    }
    return colour_out ? fail(SMX_ERR_INVALID_ARG, "%s: %s", fn, colour_text) : SMX_OK;
}

// Selects the device, runs `launch` (which returns a status if it makes a HIP call of its own) and checks the launch.
template <class F> static int launch_on(int device_id, F &&launch) {
    DeviceGuard guard(device_id);
    if (!guard.ok) return fail(SMX_ERR_HIP, "cannot select HIP device %d", device_id);
    if constexpr (std::is_void_v<decltype(launch())>) launch();
    else if (int rc = launch()) return rc;
    SMX_HIP(hipGetLastError());
    return SMX_OK;
}

// The checks shared by smx_filter_speckles and smx_fill_invalid (after their own scalar checks).
static int check_post_args(const char *fn, int n, int H, int W, const float *in, const float *out, void *workspace,
                           size_t workspace_bytes, void *stream) {
    if (!in || !out || !workspace) return fail(SMX_ERR_INVALID_ARG, "%s: in, out and workspace must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_workspace_bytes(fn, "smx_postprocess_workspace_bytes", workspace_bytes, post_layout(n, H, W).total))
        return rc;
    const size_t bytes = (size_t)n * H * W * sizeof(float);
    if (int rc = check_disjoint(fn, {{out != in ? in : nullptr, bytes}}, {{out, bytes}},
                                "out must not overlap in other than as the same buffer"))
        return rc;
    if (int rc = check_disjoint(fn, {{in, bytes}, {out, bytes}}, {{workspace, workspace_bytes}},
                                "the workspace must not overlap in or out"))
        return rc;
    return check_workspace_and_stream(fn, workspace, stream);
}

extern "C" {

int smx_lr_check(int device_id, int n, int H, int W, const float *left, const float *right, float *out, float max_diff,
                 float invalid, void *stream) {
    if (int rc = check_lr_scalars(max_diff, invalid)) return rc;
    if (!left || !right || !out) return fail(SMX_ERR_INVALID_ARG, "smx_lr_check: left, right and out must be non-NULL");
    if (int rc = check_map_dims("smx_lr_check", n, H, W)) return rc;
    if (int rc = check_caller_stream("smx_lr_check", stream)) return rc;
    const size_t bytes = (size_t)n * H * W * sizeof(float);
    if (int rc = check_disjoint("smx_lr_check", {{right, bytes}, {out != left ? left : nullptr, bytes}}, {{out, bytes}},
                                "out must not overlap right_disp, and overlap left_disp only as the same buffer"))
        return rc;
    return launch_on(device_id, [&] {
        smx::launch_lr_check(false, left, right, out, nullptr, n, H, W, max_diff, invalid, (hipStream_t)stream);
    });
}

size_t smx_postprocess_workspace_bytes(int n, int H, int W) {
    return map_dims_ok(n, H, W) ? post_layout(n, H, W).total : 0;
}

int smx_filter_speckles(int device_id, int n, int H, int W, const float *in, float *out, int max_speckle_size,
                        float max_diff, float invalid, void *workspace, size_t workspace_bytes, void *stream) {
    if (max_speckle_size < 0)
        return fail(SMX_ERR_INVALID_ARG, "smx_filter_speckles: max_speckle_size must be >= 0, got %d", max_speckle_size);
    if (int rc = check_lr_scalars(max_diff, invalid)) return rc;
    if (int rc = check_post_args("smx_filter_speckles", n, H, W, in, out, workspace, workspace_bytes, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_filter_speckles(n, H, W, in, out, max_speckle_size, max_diff, invalid, workspace, (hipStream_t)stream);
    });
}

int smx_fill_invalid(int device_id, int n, int H, int W, const float *in, float *out, float invalid, void *workspace,
                     size_t workspace_bytes, void *stream) {
    if (int rc = check_finite_marker(invalid)) return rc;
    if (int rc = check_post_args("smx_fill_invalid", n, H, W, in, out, workspace, workspace_bytes, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_fill_invalid(n, H, W, in, out, invalid, workspace, (hipStream_t)stream);
    });
}

size_t smx_median_workspace_bytes(int n, int H, int W) {
    return map_dims_ok(n, H, W) ? smx::median_workspace_bytes(n, H, W) : 0;
}

int smx_weighted_median(int device_id, int n, int H, int W, const float *in, const float *holes, const float *guide,
                        float *out, int radius, const uint16_t range_weight[256], const uint16_t spatial_weight[],
                        float invalid, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "smx_weighted_median";
    if (!in || !guide || !out)
        return fail(SMX_ERR_INVALID_ARG, "%s: in, guide and out must be non-NULL", fn);
    if (!range_weight || !spatial_weight)
        return fail(SMX_ERR_INVALID_ARG, "%s: range_weight and spatial_weight must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_int_range(fn, "radius", radius, 1, 15)) return rc;
    for (int k = 0; k < 256; ++k)
        if (range_weight[k] > 1023)
            return fail(SMX_ERR_INVALID_ARG, "%s: range_weight[%d] = %d is above 1023", fn, k, (int)range_weight[k]);
    for (int k = 0; k < (radius + 1) * (radius + 1); ++k)
        if (spatial_weight[k] > 1023)
            return fail(SMX_ERR_INVALID_ARG, "%s: spatial_weight[%d] = %d is above 1023", fn, k, (int)spatial_weight[k]);
    if (int rc = check_finite_marker(invalid)) return rc;
    if (int rc = check_workspace_bytes(fn, "smx_median_workspace_bytes", workspace_bytes, smx::median_workspace_bytes(n, H, W)))
        return rc;
    if (!workspace && workspace_bytes > 0)
        return fail(SMX_ERR_INVALID_ARG, "%s: workspace is NULL but workspace_bytes is %zu", fn, workspace_bytes);
    const size_t bytes = (size_t)n * H * W * sizeof(float);
    if (int rc = check_disjoint(fn, {{in, bytes}, {guide, bytes}}, {{out, bytes}}, "out must not overlap in or guide")) return rc;
    if (int rc = check_disjoint(fn, {{out != holes ? holes : nullptr, bytes}}, {{out, bytes}},
                                "out must not overlap holes other than as the same buffer"))
        return rc;
    if (workspace_bytes > 0)
        if (int rc = check_disjoint(fn, {{in, bytes}, {out, bytes}, {guide, bytes}, {holes, bytes}},
                                    {{workspace, workspace_bytes}}, "the workspace must not overlap in, holes, guide or out"))
            return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_weighted_median(n, H, W, in, holes, guide, out, radius, range_weight, spatial_weight, invalid,
                                    (hipStream_t)stream);
    });
}

size_t smx_wls_workspace_bytes(int n, int H, int W) {
    return map_dims_ok(n, H, W) ? wls_layout(n, H, W).total : 0;
}

int smx_wls_filter(int device_id, int n, int H, int W, const float *in, const float *confidence, const float *guide,
                   float *out, int num_iterations, const float lambdas[], const float range_weight[256],
                   float min_weight, float invalid, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "smx_wls_filter";
    if (!in || !guide || !out) return fail(SMX_ERR_INVALID_ARG, "%s: in, guide and out must be non-NULL", fn);
    if (!lambdas || !range_weight) return fail(SMX_ERR_INVALID_ARG, "%s: lambdas and range_weight must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_int_range(fn, "num_iterations", num_iterations, 1, 8)) return rc;
    for (int t = 0; t < num_iterations; ++t)
        if (!(std::isfinite(lambdas[t]) && lambdas[t] >= 0.0f && lambdas[t] <= 1048576.0f))
            return fail(SMX_ERR_INVALID_ARG, "%s: lambdas[%d] = %g is not finite in [0, 2^20]", fn, t, (double)lambdas[t]);
    for (int k = 0; k < 256; ++k)
        if (!(std::isfinite(range_weight[k]) && range_weight[k] >= 0.0f && range_weight[k] <= 1.0f))
            return fail(SMX_ERR_INVALID_ARG, "%s: range_weight[%d] = %g is not finite in [0, 1]", fn, k,
                        (double)range_weight[k]);
    if (int rc = check_non_negative(fn, "min_weight", min_weight)) return rc;
    if (int rc = check_finite_marker(invalid)) return rc;
    const size_t need = wls_layout(n, H, W).total;
    if (!workspace || workspace_bytes < need)
        return fail(SMX_ERR_INVALID_ARG, "%s: workspace is NULL or workspace_bytes %zu is below smx_wls_workspace_bytes = %zu",
                    fn, workspace_bytes, need);
    const size_t bytes = (size_t)n * H * W * sizeof(float);
    if (int rc = check_disjoint(fn, {{out != in ? in : nullptr, bytes}, {confidence, bytes}, {guide, bytes}}, {{out, bytes}},
                                "out must not overlap confidence or guide, and overlap in only as the same buffer"))
        return rc;
    if (int rc = check_disjoint(fn, {{in, bytes}, {out, bytes}, {guide, bytes}, {confidence, bytes}},
                                {{workspace, workspace_bytes}}, "the workspace must not overlap in, confidence, guide or out"))
        return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_wls(n, H, W, in, confidence, guide, out, num_iterations, lambdas, range_weight, min_weight, invalid,
                        workspace, (hipStream_t)stream);
    });
}

int smx_confidence_map(int device_id, int n, int H, int W, const float *left_disp, const float *right_disp,
                       const float *guide, int radius, float lr_scale, float texture_scale, float invalid,
                       float *out, void *stream) {
    const char *fn = "smx_confidence_map";
    if (!left_disp || !out) return fail(SMX_ERR_INVALID_ARG, "%s: left_disp and out must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (guide && (radius < 1 || radius > 15))
        return fail(SMX_ERR_INVALID_ARG, "%s: radius must be in 1..15 with a guide, got %d", fn, radius);
    if (int rc = check_positive(fn, "lr_scale", lr_scale)) return rc;
    if (int rc = check_positive(fn, "texture_scale", texture_scale)) return rc;
    if (int rc = check_finite_marker(invalid)) return rc;
    const size_t bytes = (size_t)n * H * W * sizeof(float);
    if (int rc = check_disjoint(fn, {{left_disp, bytes}, {right_disp, bytes}, {guide, bytes}}, {{out, bytes}},
                                "out must not overlap left_disp, right_disp or guide"))
        return rc;
    if (int rc = check_caller_stream(fn, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_confidence(n, H, W, left_disp, right_disp, guide, radius, lr_scale, texture_scale, invalid, out,
                               (hipStream_t)stream);
    });
}

int smx_temporal_filter(int device_id, int n, int H, int W, const float *disp, const float *confidence,
                        const float *guide, const float *prev_guide, float *state_disp, float *state_weight,
                        float *guide_out, float *out, int motion_radius, float motion_threshold, float decay,
                        float max_diff, float max_weight, float min_weight, float invalid, void *stream) {
    const char *fn = "smx_temporal_filter";
    if (!disp || !guide || !prev_guide || !state_disp || !state_weight || !out)
        return fail(SMX_ERR_INVALID_ARG, "%s: disp, guide, prev_guide, state_disp, state_weight and out must be non-NULL",
                    fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_int_range(fn, "motion_radius", motion_radius, 0, 7)) return rc;
    if (int rc = check_non_negative(fn, "motion_threshold", motion_threshold)) return rc;
    if (!(decay > 0.0f && decay <= 1.0f))
        return fail(SMX_ERR_INVALID_ARG, "%s: decay must be in (0, 1], got %g", fn, (double)decay);
    if (int rc = check_non_negative(fn, "max_diff", max_diff)) return rc;
    if (int rc = check_positive(fn, "max_weight", max_weight)) return rc;
    if (int rc = check_non_negative(fn, "min_weight", min_weight)) return rc;
    if (int rc = check_finite_marker(invalid)) return rc;
    const size_t bytes = (size_t)n * H * W * sizeof(float);
    const Span d{disp, bytes}, d_unless_out{out != disp ? disp : nullptr, bytes}, c{confidence, bytes}, g{guide, bytes},
        pg{prev_guide, bytes}, sd{state_disp, bytes}, sw{state_weight, bytes}, go{guide_out, bytes}, o{out, bytes};
    if (int rc = check_disjoint(fn, {d_unless_out}, {o}, "out must not overlap disp other than as the same buffer")) return rc;
    if (int rc = check_disjoint(fn, {c, g, pg, sd, sw, go}, {o}, "out must not overlap an operand other than disp")) return rc;
    if (int rc = check_disjoint(fn, {d, c, g, pg}, {sd, sw}, "the state buffers must not overlap an input")) return rc;
    if (int rc = check_disjoint(fn, {sd}, {sw}, "state_disp and state_weight overlap")) return rc;
    if (int rc = check_disjoint(fn, {d, c, g, pg, sd, sw}, {go}, "guide_out must not overlap another operand")) return rc;
    if (int rc = check_caller_stream(fn, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_temporal(n, H, W, disp, confidence, guide, prev_guide, state_disp, state_weight, guide_out, out,
                             motion_radius, motion_threshold, decay, max_diff, max_weight, min_weight, invalid,
                             (hipStream_t)stream);
    });
}

int smx_remap_pairs(int device_id, int n, int channels, int dtype, int H_in, int W_in, int H_out, int W_out,
                    const void *left_in, const void *right_in, const int32_t *left_map, const int32_t *right_map,
                    void *left_out, void *right_out, int border_mode, float border_value, void *stream) {
    const char *fn = "smx_remap_pairs";
    if (!left_in || !left_map || !left_out)
        return fail(SMX_ERR_INVALID_ARG, "%s: left_in, left_map and left_out must be non-NULL", fn);
    const int right_set = (right_in != nullptr) + (right_map != nullptr) + (right_out != nullptr);
    if (right_set != 0 && right_set != 3)
        return fail(SMX_ERR_INVALID_ARG, "%s: right_in, right_map and right_out must be all NULL or all non-NULL", fn);
    if (n < 1) return fail(SMX_ERR_INVALID_ARG, "%s: need n >= 1, got %d", fn, n);
    if (H_in < 1 || W_in < 1 || H_out < 1 || W_out < 1 || H_in > 32768 || W_in > 32768 || H_out > 32768 || W_out > 32768)
        return fail(SMX_ERR_INVALID_ARG, "%s: sizes must be in 1..32768 (got in %dx%d, out %dx%d)", fn, H_in, W_in, H_out,
                    W_out);
    if (int rc = check_int_range(fn, "channels", channels, 1, 4)) return rc;
    if (int rc = check_dtype(fn, "", dtype)) return rc;
    if (border_mode != SMX_BORDER_CONSTANT && border_mode != SMX_BORDER_REPLICATE)
        return fail(SMX_ERR_INVALID_ARG, "%s: unknown border mode %d", fn, border_mode);
    if (!std::isfinite(border_value))
        return fail(SMX_ERR_INVALID_ARG, "%s: border_value must be finite, got %g", fn, (double)border_value);
    if (dtype == SMX_DTYPE_U8 && !(border_value >= 0.0f && border_value <= 255.0f && border_value == std::floor(border_value)))
        return fail(SMX_ERR_INVALID_ARG, "%s: a uint8 border_value must be an integer in 0..255, got %g", fn,
                    (double)border_value);
    const size_t es = dtype == SMX_DTYPE_F32 ? 4 : 1;
    const size_t frame = (size_t)channels * (size_t)(H_in > H_out ? H_in : H_out) * (size_t)(W_in > W_out ? W_in : W_out) * es;
    if ((size_t)n > SIZE_MAX / frame)                       // frame < 2^34: the byte sizes below do not overflow
        return fail(SMX_ERR_INVALID_ARG, "%s: n = %d frames do not fit the address space", fn, n);
    const size_t in_bytes = (size_t)n * channels * H_in * W_in * es;
    const size_t out_bytes = (size_t)n * channels * H_out * W_out * es;
    const size_t map_bytes = (size_t)H_out * W_out * 2 * sizeof(int32_t);
    if (int rc = check_disjoint(fn, {{left_in, in_bytes}, {right_in, in_bytes}, {left_map, map_bytes}, {right_map, map_bytes}},
                                {{left_out, out_bytes}, {right_out, out_bytes}}, "an output overlaps an input or a map"))
        return rc;
    if (int rc = check_disjoint(fn, {{left_out, out_bytes}}, {{right_out, out_bytes}}, "left_out and right_out overlap")) return rc;
    if (int rc = check_caller_stream(fn, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_remap_pairs(n, channels, dtype == SMX_DTYPE_F32, H_in, W_in, H_out, W_out, left_in, right_in, left_map,
                                right_map, left_out, right_out, border_mode == SMX_BORDER_REPLICATE, border_value,
                                (hipStream_t)stream);
    });
}

// The rules the three entries of the synthesis head share, in their order.  vol: the [n][D][h][w] operand (prob or
// grad_prob), img: the second [n][C][H][W] f32 operand (out, view or grad_view); out_is_vol: which of the two is written.
static int check_synthesis_args(const char *fn, int n, int channels, int dtype, int D, int h, int w, int scale,
                                const void *vol, const char *vol_name, const void *left, const void *img,
                                const char *img_name, bool out_is_vol, void *stream) {
    if (!vol || !left || !img) {
        const char *first = out_is_vol ? img_name : vol_name, *last = out_is_vol ? vol_name : img_name;
        return fail(SMX_ERR_INVALID_ARG, "%s: %s, left and %s must be non-NULL", fn, first, last);
    }
    if (n < 1) return fail(SMX_ERR_INVALID_ARG, "%s: need n >= 1, got %d", fn, n);
    if (channels != 1 && channels != 3) return fail(SMX_ERR_INVALID_ARG, "%s: channels must be 1 or 3, got %d", fn, channels);
    if (int rc = check_dtype(fn, "", dtype)) return rc;
    if (int rc = check_int_range(fn, "D", D, 1, 256)) return rc;
    if (int rc = check_int_range(fn, "scale", scale, 1, 16)) return rc;
    if (h < 1 || w < 1 || h > 32768 / scale || w > 32768 / scale)
        return fail(SMX_ERR_INVALID_ARG, "%s: need h, w >= 1 and h * scale, w * scale <= 32768 (got h %d, w %d, scale %d)", fn,
                    h, w, scale);
    const size_t px = (size_t)h * scale * w * scale;                        // <= 2^30
    const size_t frame = ((size_t)D * h * w > px * channels ? (size_t)D * h * w : px * channels) * sizeof(float);
    if ((size_t)n > SIZE_MAX / frame)                                       // frame <= 2^40: the byte sizes below do not overflow
        return fail(SMX_ERR_INVALID_ARG, "%s: n = %d frames do not fit the address space", fn, n);
    const Span v{vol, (size_t)n * D * h * w * sizeof(float)}, i{img, (size_t)n * channels * px * sizeof(float)};
    const Span l{left, (size_t)n * channels * px * (dtype == SMX_DTYPE_F32 ? 4 : 1)};
    char text[96];
    if (out_is_vol) snprintf(text, sizeof text, "%s must not overlap %s or left", vol_name, img_name);
    else snprintf(text, sizeof text, "%s must not overlap %s or left", img_name, vol_name);
    if (int rc = out_is_vol ? check_disjoint(fn, {i, l}, {v}, text) : check_disjoint(fn, {v, l}, {i}, text)) return rc;
    return check_caller_stream(fn, stream);
}

int smx_synthesize_right_view(int device_id, int n, int channels, int dtype, int D, int h, int w, int scale,
                              const float *prob, const void *left, float *out, void *stream) {
    if (int rc = check_synthesis_args("smx_synthesize_right_view", n, channels, dtype, D, h, w, scale, prob, "prob", left, out,
                                      "out", false, stream))
        return rc;
    return launch_on(device_id, [&] {
        smx::launch_synthesis(n, channels, dtype == SMX_DTYPE_F32, D, h, w, scale, prob, left, out, (hipStream_t)stream);
    });
}

int smx_synthesis_head_forward(int device_id, int n, int channels, int dtype, int D, int h, int w, int scale,
                               const float *prob, const void *left, float *view, void *stream) {
    if (int rc = check_synthesis_args("smx_synthesis_head_forward", n, channels, dtype, D, h, w, scale, prob, "prob", left, view,
                                      "view", false, stream))
        return rc;
    return launch_on(device_id, [&] {
        smx::launch_synthesis_view(n, channels, dtype == SMX_DTYPE_F32, D, h, w, scale, prob, left, view, (hipStream_t)stream);
    });
}

int smx_synthesis_head_backward(int device_id, int n, int channels, int dtype, int D, int h, int w, int scale,
                                const float *grad_view, const void *left, float *grad_prob, void *stream) {
    if (int rc = check_synthesis_args("smx_synthesis_head_backward", n, channels, dtype, D, h, w, scale, grad_prob, "grad_prob",
                                      left, grad_view, "grad_view", true, stream))
        return rc;
    return launch_on(device_id, [&] {
        smx::launch_synthesis_grad(n, channels, dtype == SMX_DTYPE_F32, D, h, w, scale, grad_view, left, grad_prob,
                                   (hipStream_t)stream);
    });
}

// The size rules of smx_sgm that the workspace query shares: 0 = accepted.
static int sgm_size_error(int n, int H, int W, int D, int paths) {
    if (!map_dims_ok(n, H, W)) return 1;
    if (D < 1 || D > 256) return 2;
    if (paths != 4 && paths != 8) return 3;
    if ((size_t)n * (size_t)(H + W) > ((size_t)1 << 31)) return 4;
    return 0;
}

size_t smx_sgm_workspace_bytes(int n, int H, int W, int num_disparities, int paths) {
    return sgm_size_error(n, H, W, num_disparities, paths) ? 0 : sgm_layout(n, H, W, num_disparities).total;
}

// smx_sgm and smx_sgm_with_right_map: right_out NULL is smx_sgm.
static int sgm_entry(const char *fn, int device_id, int n, int channels, int dtype, int H, int W, const void *left,
                     const void *right, int min_disparity, int num_disparities, int paths, int P1, int P2,
                     int uniqueness, float lr_max_diff, int subpixel, float invalid_disparity, float *out,
                     float *gray_left_out, float *right_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!left || !right || !out || !workspace)
        return fail(SMX_ERR_INVALID_ARG, "%s: left, right, out and workspace must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if ((size_t)n * (size_t)(H + W) > ((size_t)1 << 31))
        return fail(SMX_ERR_INVALID_ARG, "%s: n * (H + W) = %zu exceeds 2^31: split the batch", fn,
                    (size_t)n * (size_t)(H + W));
    if (channels != 1 && channels != 3) return fail(SMX_ERR_INVALID_ARG, "%s: channels must be 1 or 3, got %d", fn, channels);
    if (int rc = check_dtype(fn, "", dtype)) return rc;
    if (int rc = check_int_range(fn, "min_disparity", min_disparity, 0, 32768)) return rc;
    if (int rc = check_int_range(fn, "num_disparities", num_disparities, 1, 256)) return rc;
    if (paths != 4 && paths != 8) return fail(SMX_ERR_INVALID_ARG, "%s: paths must be 4 or 8, got %d", fn, paths);
    if (!(0 <= P1 && P1 <= P2 && P2 <= 191))
        return fail(SMX_ERR_INVALID_ARG, "%s: need 0 <= P1 <= P2 <= 191, got P1 %d, P2 %d", fn, P1, P2);
    if (uniqueness < 0 || uniqueness > 99)
        return fail(SMX_ERR_INVALID_ARG, "%s: uniqueness must be in 0..99 (percent, 0: off), got %d", fn, uniqueness);
    if (!std::isfinite(lr_max_diff))
        return fail(SMX_ERR_INVALID_ARG, "%s: lr_max_diff must be finite (negative: no LR check), got %g", fn,
                    (double)lr_max_diff);
    if (int rc = check_finite_marker(invalid_disparity)) return rc;
    if (int rc = check_workspace_bytes(fn, "smx_sgm_workspace_bytes", workspace_bytes,
                                       sgm_layout(n, H, W, num_disparities).total))
        return rc;
    const size_t in_bytes = (size_t)n * channels * H * W * (dtype == SMX_DTYPE_F32 ? 4 : 1);
    const size_t map_bytes = (size_t)n * H * W * sizeof(float);
    const Span l{left, in_bytes}, r{right, in_bytes}, ws{workspace, workspace_bytes}, o{out, map_bytes},
        g{gray_left_out, map_bytes}, ro{right_out, map_bytes};
    if (int rc = check_disjoint(fn, {l, r, ws}, {o, g, ro}, "the outputs must not overlap left, right or the workspace")) return rc;
    if (int rc = check_disjoint(fn, {g}, {o}, "out and gray_left_out overlap")) return rc;
    if (int rc = check_disjoint(fn, {o, g}, {ro}, "right_out overlaps out or gray_left_out")) return rc;
    if (int rc = check_disjoint(fn, {l, r}, {ws}, "the workspace must not overlap left or right")) return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_sgm(n, channels, dtype == SMX_DTYPE_F32, H, W, left, right, min_disparity, num_disparities, paths, P1,
                        P2, uniqueness, lr_max_diff, subpixel != 0, invalid_disparity, out, gray_left_out, right_out,
                        workspace, (hipStream_t)stream);
    });
}

int smx_sgm(int device_id, int n, int channels, int dtype, int H, int W, const void *left, const void *right,
            int min_disparity, int num_disparities, int paths, int P1, int P2, int uniqueness, float lr_max_diff,
            int subpixel, float invalid_disparity, float *out, float *gray_left_out, void *workspace,
            size_t workspace_bytes, void *stream) {
    return sgm_entry("smx_sgm", device_id, n, channels, dtype, H, W, left, right, min_disparity, num_disparities, paths,
                     P1, P2, uniqueness, lr_max_diff, subpixel, invalid_disparity, out, gray_left_out, nullptr,
                     workspace, workspace_bytes, stream);
}

int smx_sgm_with_right_map(int device_id, int n, int channels, int dtype, int H, int W, const void *left,
                           const void *right, int min_disparity, int num_disparities, int paths, int P1, int P2,
                           int uniqueness, float lr_max_diff, int subpixel, float invalid_disparity, float *out,
                           float *gray_left_out, float *right_out, void *workspace, size_t workspace_bytes,
                           void *stream) {
    const char *fn = "smx_sgm_with_right_map";
    if (!right_out) return fail(SMX_ERR_INVALID_ARG, "%s: right_out must be non-NULL", fn);
    return sgm_entry(fn, device_id, n, channels, dtype, H, W, left, right, min_disparity, num_disparities, paths, P1, P2,
                     uniqueness, lr_max_diff, subpixel, invalid_disparity, out, gray_left_out, right_out, workspace,
                     workspace_bytes, stream);
}

int smx_disparity_to_points(int device_id, const float *disp, int H, int W, float bf, float invalid,
                            float *depth, float *points, int *count_dev, int *workspace, void *stream) {
    if (!disp || !points || !count_dev || !workspace || H < 1 || W < 1 || H > 32768)
        return fail(SMX_ERR_INVALID_ARG, "smx_disparity_to_points: NULL pointer or bad size");
    return launch_on(device_id, [&] {
        smx::launch_points(disp, H, W, bf, invalid, depth, points, count_dev, workspace, (hipStream_t)stream);
    });
}

int smx_eval_metrics(int device_id, int n, const float *est, const float *gt, const uint8_t *mask,
                     size_t pixels, float max_disparity, const float thresholds[4], double *out_sums,
                     void *stream) {
    if (!est || !gt || !out_sums || !thresholds || n < 1 || pixels == 0)
        return fail(SMX_ERR_INVALID_ARG, "smx_eval_metrics: NULL pointer, n < 1 or no pixels");
    return launch_on(device_id, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        SMX_HIP(hipMemsetAsync(out_sums, 0, sizeof(double) * 8 * (size_t)n, s));
        smx::launch_metrics(n, est, gt, mask, pixels, max_disparity, thresholds, out_sums, s);
        return SMX_OK;
    });
}

// ---- metric 3D points ----------------------------------------------------------------------------------------------------
size_t smx_reproject_workspace_bytes(int n, int H, int W) {
    return points_dims_ok(n, H, W) ? reproject_layout(n, H).total : 0;
}

int smx_reproject_points(int device_id, int n, int H, int W, const float *disp, const float Q[16],
                         const float *confidence, float min_confidence, float z_min, float z_max,
                         float invalid_disparity, const void *image, int image_channels, int image_dtype,
                         float *points, uint8_t *colors, int32_t *indices, float *xyz_map, int32_t *offsets,
                         void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "smx_reproject_points";
    if (!disp || !Q || !points || !offsets || !workspace)
        return fail(SMX_ERR_INVALID_ARG, "%s: disp, Q, points, offsets and workspace must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_pixel_count(fn, n, H, W)) return rc;
    if (int rc = check_finite_array(fn, "Q", Q, 16)) return rc;
    if (int rc = check_reprojection_args(fn, z_min, z_max, min_confidence, invalid_disparity, image, image_channels,
                                         image_dtype, colors, "colors needs an image"))
        return rc;
    if (int rc = check_workspace_bytes(fn, "smx_reproject_workspace_bytes", workspace_bytes, reproject_layout(n, H).total))
        return rc;
    const size_t px = (size_t)n * H * W;
    const size_t map_bytes = px * sizeof(float);
    const size_t img_bytes = image ? px * image_channels * (image_dtype == SMX_DTYPE_F32 ? 4 : 1) : 0;
    if (int rc = check_disjoint(fn, {{disp, map_bytes}, {confidence, map_bytes}, {image, img_bytes}, {workspace, workspace_bytes}},
                                {{points, px * 3 * sizeof(float)}, {colors, px * 3}, {indices, px * sizeof(int32_t)},
                                 {xyz_map, px * 3 * sizeof(float)}, {offsets, ((size_t)n + 1) * sizeof(int32_t)}},
                                "an output overlaps an input or the workspace", "two outputs overlap"))
        return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_reproject(n, H, W, disp, Q, confidence, min_confidence, z_min, z_max, invalid_disparity, image,
                              image_channels, image_dtype == SMX_DTYPE_F32, points, colors, indices, xyz_map, offsets,
                              workspace, (hipStream_t)stream);
    });
}

static bool voxel_dims_ok(int n, int capacity) { return n >= 1 && n <= 65536 && capacity >= 1 && capacity <= SMX_POINTS_MAX; }

size_t smx_voxel_workspace_bytes(int n, int capacity) {
    return voxel_dims_ok(n, capacity) ? vox_layout(n, capacity).total : 0;
}

int smx_voxel_downsample(int device_id, int n, int capacity, const float *points, const uint8_t *colors,
                         const int32_t *offsets, float voxel_size, int min_points, float *out_points,
                         uint8_t *out_colors, int32_t *out_counts, int32_t *out_offsets, int32_t *dropped,
                         void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "smx_voxel_downsample";
    if (!points || !offsets || !out_points || !out_counts || !out_offsets || !dropped || !workspace)
        return fail(SMX_ERR_INVALID_ARG,
                    "%s: points, offsets, out_points, out_counts, out_offsets, dropped and workspace must be non-NULL", fn);
    if ((colors == nullptr) != (out_colors == nullptr))
        return fail(SMX_ERR_INVALID_ARG, "%s: colors and out_colors must be both NULL or both non-NULL", fn);
    if (!voxel_dims_ok(n, capacity))
        return fail(SMX_ERR_INVALID_ARG, "%s: need 1 <= n <= 65536 and 1 <= capacity <= 2^30 (got n %d, capacity %d)", fn,
                    n, capacity);
    if (int rc = check_positive(fn, "voxel_size", voxel_size)) return rc;
    if (min_points < 1) return fail(SMX_ERR_INVALID_ARG, "%s: min_points must be >= 1, got %d", fn, min_points);
    if (int rc = check_workspace_bytes(fn, "smx_voxel_workspace_bytes", workspace_bytes, vox_layout(n, capacity).total))
        return rc;
    const size_t cap = (size_t)capacity, offs = ((size_t)n + 1) * sizeof(int32_t);
    const size_t xyz = cap * 3 * sizeof(float);
    if (int rc = check_disjoint(fn, {{points, xyz}, {colors, cap * 3}, {offsets, offs}, {workspace, workspace_bytes}},
                                {{out_points, xyz}, {out_colors, cap * 3}, {out_counts, cap * sizeof(int32_t)},
                                 {out_offsets, offs}, {dropped, (size_t)n * sizeof(int32_t)}},
                                "an output overlaps an input or the workspace", "two outputs overlap"))
        return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&]() -> int {
        SMX_HIP(smx::launch_voxel_downsample(n, capacity, points, colors, offsets, voxel_size, min_points, out_points,
                                             out_colors, out_counts, out_offsets, dropped, workspace,
                                             (hipStream_t)stream));
        return SMX_OK;
    });
}

// ---- point clouds back into camera views -------------------------------------------------------------------------------
static bool project_dims_ok(int n, int H, int W) { return n <= 65536 && points_dims_ok(n, H, W); }

size_t smx_project_workspace_bytes(int n, int H, int W) {
    return project_dims_ok(n, H, W) ? project_layout(n, H, W).total : 0;
}

int smx_project_points(int device_id, int n, int capacity, int H, int W, const float *points, const int32_t *offsets,
                       const float *world_to_camera, const float P[16], int radius, float z_min, float z_max,
                       float invalid_disparity, float *disp, int32_t *index, float *depth, void *workspace,
                       size_t workspace_bytes, void *stream) {
    const char *fn = "smx_project_points";
    if (!points || !offsets || !world_to_camera || !P || !disp || !workspace)
        return fail(SMX_ERR_INVALID_ARG, "%s: points, offsets, world_to_camera, P, disp and workspace must be non-NULL", fn);
    if (!voxel_dims_ok(n, capacity))
        return fail(SMX_ERR_INVALID_ARG, "%s: need 1 <= n <= 65536 and 1 <= capacity <= 2^30 (got n %d, capacity %d)", fn,
                    n, capacity);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_pixel_count(fn, n, H, W)) return rc;
    if (int rc = check_int_range(fn, "radius", radius, 0, 8)) return rc;
    if (int rc = check_finite_array(fn, "P", P, 16)) return rc;
    if (int rc = check_reprojection_args(fn, z_min, z_max, 0.0f, invalid_disparity, nullptr, 0, 0, nullptr, "")) return rc;
    if (int rc = check_workspace_bytes(fn, "smx_project_workspace_bytes", workspace_bytes, project_layout(n, H, W).total))
        return rc;
    const size_t plane = (size_t)n * H * W * sizeof(float);
    if (int rc = check_disjoint(fn, {{points, (size_t)capacity * 3 * sizeof(float)}, {offsets, ((size_t)n + 1) * sizeof(int32_t)},
                                     {world_to_camera, (size_t)n * 12 * sizeof(float)}},
                                {{disp, plane}, {index, plane}, {depth, plane}, {workspace, workspace_bytes}},
                                "an output or the workspace overlaps an input", "two outputs (or one and the workspace) overlap"))
        return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_project(n, capacity, H, W, points, offsets, world_to_camera, P, radius, z_min, z_max,
                            invalid_disparity, disp, index, depth, workspace, (hipStream_t)stream);
    });
}

// ---- TSDF fusion -------------------------------------------------------------------------------------------------------
static constexpr long SMX_TSDF_VOXELS_MAX = 1L << 30;

static bool tsdf_dims_ok(int nx, int ny, int nz) {
    return nx >= 1 && ny >= 1 && nz >= 1 && nx <= 4096 && ny <= 4096 && nz <= 4096 &&
           (long)nx * ny * nz <= SMX_TSDF_VOXELS_MAX;
}

static int check_tsdf_dims(const char *fn, int nx, int ny, int nz) {
    if (tsdf_dims_ok(nx, ny, nz)) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "%s: need 1 <= nx, ny, nz <= 4096 and nx * ny * nz <= 2^30 (got %d, %d, %d)", fn, nx,
                ny, nz);
}

// The volume's checks shared by smx_tsdf_integrate and smx_tsdf_extract_points (after their NULL checks).
static int check_tsdf_volume(const char *fn, int nx, int ny, int nz, const float origin[3], float voxel_size) {
    if (int rc = check_tsdf_dims(fn, nx, ny, nz)) return rc;
    if (int rc = check_positive(fn, "voxel_size", voxel_size)) return rc;
    return check_finite_array(fn, "origin", origin, 3);
}

// The texts of the TSDF entries' disjointness rule.
static const char *const TSDF_IN_TEXT = "an output or the workspace overlaps an input";
static const char *const TSDF_OUT_TEXT = "two outputs (state arrays, workspace) overlap";

size_t smx_tsdf_integrate_workspace_bytes(int n, int H, int W) {
    return points_dims_ok(n, H, W) ? tsdf_integrate_layout(n, H, W).total : 0;
}

int smx_tsdf_integrate(int device_id, int nx, int ny, int nz, const float origin[3], float voxel_size,
                       float truncation, float max_weight, float *tsdf, float *weight, uint8_t *color, int n, int H,
                       int W, const float *disp, const float Q[16], const float P[16], const float *world_to_camera,
                       const float *confidence, float min_confidence, float z_min, float z_max,
                       float invalid_disparity, const void *image, int image_channels, int image_dtype,
                       void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "smx_tsdf_integrate";
    if (!origin || !tsdf || !weight || !disp || !Q || !P || !world_to_camera || !workspace)
        return fail(SMX_ERR_INVALID_ARG,
                    "%s: origin, tsdf, weight, disp, Q, P, world_to_camera and workspace must be non-NULL", fn);
    if (int rc = check_tsdf_volume(fn, nx, ny, nz, origin, voxel_size)) return rc;
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_pixel_count(fn, n, H, W)) return rc;
    if (!(std::isfinite(truncation) && truncation > voxel_size))
        return fail(SMX_ERR_INVALID_ARG, "%s: truncation must be finite and > voxel_size, got %g", fn, (double)truncation);
    if (int rc = check_positive(fn, "max_weight", max_weight)) return rc;
    for (int k = 0; k < 16; ++k) {                            // one loop: the lower index is reported, Q before P
        if (int rc = check_finite_at(fn, "Q", Q, k)) return rc;
        if (int rc = check_finite_at(fn, "P", P, k)) return rc;
    }
    if (int rc = check_reprojection_args(fn, z_min, z_max, min_confidence, invalid_disparity, image, image_channels,
                                         image_dtype, color, "a colour volume needs an image"))
        return rc;
    if (int rc = check_workspace_bytes(fn, "smx_tsdf_integrate_workspace_bytes", workspace_bytes,
                                       tsdf_integrate_layout(n, H, W).total))
        return rc;
    const size_t vox = (size_t)nx * ny * nz, px = (size_t)n * H * W, map_bytes = px * sizeof(float);
    const size_t img_bytes = image ? px * image_channels * (image_dtype == SMX_DTYPE_F32 ? 4 : 1) : 0;
    if (int rc = check_disjoint(fn, {{disp, map_bytes}, {confidence, map_bytes}, {image, img_bytes},
                                     {world_to_camera, (size_t)n * 12 * sizeof(float)}},
                                {{tsdf, vox * sizeof(float)}, {weight, vox * sizeof(float)}, {color, vox * 4},
                                 {workspace, workspace_bytes}}, TSDF_IN_TEXT, TSDF_OUT_TEXT))
        return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_tsdf_integrate(nx, ny, nz, origin, voxel_size, truncation, max_weight, tsdf, weight, color, n, H, W,
                                   disp, Q, P, world_to_camera, confidence, min_confidence, z_min, z_max,
                                   invalid_disparity, image, image_channels, image_dtype == SMX_DTYPE_F32, workspace,
                                   (hipStream_t)stream);
    });
}

size_t smx_tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
    return tsdf_dims_ok(nx, ny, nz) ? tsdf_extract_layout(ny, nz).total : 0;
}

int smx_tsdf_extract_points(int device_id, int nx, int ny, int nz, const float origin[3], float voxel_size,
                            const float *tsdf, const float *weight, const uint8_t *color, float min_weight,
                            int capacity, float *points, float *normals, uint8_t *colors, int32_t *count,
                            void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "smx_tsdf_extract_points";
    if (!origin || !tsdf || !weight || !points || !count || !workspace)
        return fail(SMX_ERR_INVALID_ARG, "%s: origin, tsdf, weight, points, count and workspace must be non-NULL", fn);
    if (int rc = check_tsdf_volume(fn, nx, ny, nz, origin, voxel_size)) return rc;
    if (int rc = check_positive(fn, "min_weight", min_weight)) return rc;
    if (int rc = check_capacity(fn, capacity)) return rc;
    if (colors && !color) return fail(SMX_ERR_INVALID_ARG, "%s: colors needs a colour volume", fn);
    if (int rc = check_workspace_bytes(fn, "smx_tsdf_extract_workspace_bytes", workspace_bytes,
                                       tsdf_extract_layout(ny, nz).total))
        return rc;
    const size_t vox = (size_t)nx * ny * nz, cap = (size_t)capacity;
    if (int rc = check_disjoint(fn, {{tsdf, vox * sizeof(float)}, {weight, vox * sizeof(float)}, {color, vox * 4}},
                                {{points, cap * 3 * sizeof(float)}, {normals, cap * 3 * sizeof(float)}, {colors, cap * 3},
                                 {count, sizeof(int32_t)}, {workspace, workspace_bytes}}, TSDF_IN_TEXT, TSDF_OUT_TEXT))
        return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_tsdf_extract(nx, ny, nz, origin, voxel_size, tsdf, weight, color, min_weight, capacity, points,
                                 normals, colors, count, workspace, (hipStream_t)stream);
    });
}

size_t smx_tsdf_extract_triangles_workspace_bytes(int nx, int ny, int nz) {
    return tsdf_dims_ok(nx, ny, nz) ? mesh_layout(nx, ny, nz).total : 0;
}

int smx_tsdf_extract_triangles(int device_id, int nx, int ny, int nz, const float *tsdf, const float *weight,
                               float min_weight, int capacity, int32_t *triangles, int32_t *count, void *workspace,
                               size_t workspace_bytes, void *stream) {
    const char *fn = "smx_tsdf_extract_triangles";
    if (!tsdf || !weight || !triangles || !count || !workspace)
        return fail(SMX_ERR_INVALID_ARG, "%s: tsdf, weight, triangles, count and workspace must be non-NULL", fn);
    if (int rc = check_tsdf_dims(fn, nx, ny, nz)) return rc;
    if (int rc = check_positive(fn, "min_weight", min_weight)) return rc;
    if (int rc = check_capacity(fn, capacity)) return rc;
    if (int rc = check_workspace_bytes(fn, "smx_tsdf_extract_triangles_workspace_bytes", workspace_bytes,
                                       mesh_layout(nx, ny, nz).total))
        return rc;
    const size_t vox = (size_t)nx * ny * nz;
    if (int rc = check_disjoint(fn, {{tsdf, vox * sizeof(float)}, {weight, vox * sizeof(float)}},
                                {{triangles, (size_t)capacity * 3 * sizeof(int32_t)}, {count, sizeof(int32_t)},
                                 {workspace, workspace_bytes}}, TSDF_IN_TEXT, TSDF_OUT_TEXT))
        return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_tsdf_triangles(nx, ny, nz, tsdf, weight, min_weight, capacity, triangles, count, workspace,
                                   (hipStream_t)stream);
    });
}

size_t smx_tsdf_raycast_workspace_bytes(int nx, int ny, int nz) {
    return tsdf_dims_ok(nx, ny, nz) ? raycast_layout(nx, ny, nz).total : 0;
}

int smx_tsdf_raycast(int device_id, int nx, int ny, int nz, const float origin[3], float voxel_size,
                     const float *tsdf, const float *weight, const uint8_t *color, float min_weight, int n, int H,
                     int W, const float Q[16], const float *camera_to_world, float step, float z_min, float z_max,
                     float invalid_disparity, float *disp, float *depth, float *normals, uint8_t *colors,
                     float *out_weight, void *workspace, size_t workspace_bytes, void *stream) {
    const char *fn = "smx_tsdf_raycast";
    if (!origin || !tsdf || !weight || !Q || !camera_to_world || !disp || !workspace)
        return fail(SMX_ERR_INVALID_ARG,
                    "%s: origin, tsdf, weight, Q, camera_to_world, disp and workspace must be non-NULL", fn);
    if (int rc = check_tsdf_volume(fn, nx, ny, nz, origin, voxel_size)) return rc;
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_pixel_count(fn, n, H, W)) return rc;
    if (int rc = check_positive(fn, "min_weight", min_weight)) return rc;
    if (int rc = check_positive(fn, "step", step)) return rc;
    if (!(std::isfinite(z_min) && std::isfinite(z_max) && z_min >= 0.0f && z_min <= z_max))
        return fail(SMX_ERR_INVALID_ARG, "%s: need finite 0 <= z_min <= z_max, got %g, %g", fn, (double)z_min,
                    (double)z_max);
    const float samples = floorf((z_max - z_min) / step);            // M - 1, in the header's float32 steps
    if (!(samples >= 0.0f && samples <= 65535.0f))
        return fail(SMX_ERR_INVALID_ARG, "%s: (z_max - z_min) / step gives %g samples per ray, the limit is 65536", fn,
                    (double)samples + 1.0);
    if (int rc = check_finite_array(fn, "Q", Q, 16)) return rc;
    if (Q[2] != 0.0f || Q[6] != 0.0f || Q[10] != 0.0f || Q[12] != 0.0f || Q[13] != 0.0f || Q[14] == 0.0f)
        return fail(SMX_ERR_INVALID_ARG,
                    "%s: Q's ray must not depend on d: need Q02 = Q12 = Q22 = 0, Q30 = Q31 = 0 and Q32 != 0", fn);
    if (!std::isfinite(invalid_disparity))
        return fail(SMX_ERR_INVALID_ARG, "%s: invalid_disparity must be finite, got %g", fn, (double)invalid_disparity);
    if (colors && !color) return fail(SMX_ERR_INVALID_ARG, "%s: colors needs a colour volume", fn);
    if (int rc = check_workspace_bytes(fn, "smx_tsdf_raycast_workspace_bytes", workspace_bytes,
                                       raycast_layout(nx, ny, nz).total))
        return rc;
    const size_t vox = (size_t)nx * ny * nz, px = (size_t)n * H * W;
    if (int rc = check_disjoint(fn, {{tsdf, vox * sizeof(float)}, {weight, vox * sizeof(float)}, {color, vox * 4},
                                     {camera_to_world, (size_t)n * 12 * sizeof(float)}},
                                {{disp, px * sizeof(float)}, {depth, px * sizeof(float)},
                                 {normals, px * 3 * sizeof(float)}, {colors, px * 3}, {out_weight, px * sizeof(float)},
                                 {workspace, workspace_bytes}}, TSDF_IN_TEXT, TSDF_OUT_TEXT))
        return rc;
    if (int rc = check_workspace_and_stream(fn, workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_tsdf_raycast(nx, ny, nz, origin, voxel_size, tsdf, weight, color, min_weight, n, H, W, Q,
                                 camera_to_world, step, z_min, (int)samples + 1, invalid_disparity, disp, depth, normals,
                                 colors, out_weight, workspace, (hipStream_t)stream);
    });
}

int smx_tsdf_window(int device_id, int nx, int ny, int nz, const float *tsdf, const float *weight, const uint8_t *color,
                    int x0, int y0, int z0, int bx, int by, int bz, float *tsdf_out, float *weight_out,
                    uint8_t *color_out, void *stream) {
    const char *fn = "smx_tsdf_window";
    if (!tsdf || !weight || !tsdf_out || !weight_out)
        return fail(SMX_ERR_INVALID_ARG, "%s: tsdf, weight, tsdf_out and weight_out must be non-NULL", fn);
    if ((color == nullptr) != (color_out == nullptr))
        return fail(SMX_ERR_INVALID_ARG, "%s: color and color_out must both be NULL or both be given", fn);
    if (int rc = check_tsdf_dims(fn, nx, ny, nz)) return rc;
    if (!tsdf_dims_ok(bx, by, bz))
        return fail(SMX_ERR_INVALID_ARG, "%s: need 1 <= bx, by, bz <= 4096 and bx * by * bz <= 2^30 (got %d, %d, %d)", fn, bx,
                    by, bz);
    if (int rc = check_int_range(fn, "x0", x0, -8192, 8192)) return rc;
    if (int rc = check_int_range(fn, "y0", y0, -8192, 8192)) return rc;
    if (int rc = check_int_range(fn, "z0", z0, -8192, 8192)) return rc;
    const size_t vox = (size_t)nx * ny * nz, out = (size_t)bx * by * bz;
    if (int rc = check_disjoint(fn, {{tsdf, vox * sizeof(float)}, {weight, vox * sizeof(float)}, {color, vox * 4}},
                                {{tsdf_out, out * sizeof(float)}, {weight_out, out * sizeof(float)}, {color_out, out * 4}},
                                "a destination array overlaps a source array (the call is out of place)",
                                "two destination arrays overlap"))
        return rc;
    if (int rc = check_caller_stream(fn, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_tsdf_window(nx, ny, nz, tsdf, weight, color, x0, y0, z0, bx, by, bz, tsdf_out, weight_out, color_out,
                                (hipStream_t)stream);
    });
}

int smx_tsdf_merge(int device_id, int nx, int ny, int nz, float *tsdf, float *weight, uint8_t *color, int sx, int sy,
                   int sz, const float *src_tsdf, const float *src_weight, const uint8_t *src_color, int x0, int y0, int z0,
                   int rx, int ry, int rz, int cx, int cy, int cz, int mode, float max_weight, void *stream) {
    const char *fn = "smx_tsdf_merge";
    if (!tsdf || !weight || !src_tsdf || !src_weight)
        return fail(SMX_ERR_INVALID_ARG, "%s: tsdf, weight, src_tsdf and src_weight must be non-NULL", fn);
    if ((color == nullptr) != (src_color == nullptr))
        return fail(SMX_ERR_INVALID_ARG, "%s: color and src_color must both be NULL or both be given", fn);
    if (int rc = check_tsdf_dims(fn, nx, ny, nz)) return rc;
    if (!tsdf_dims_ok(sx, sy, sz))
        return fail(SMX_ERR_INVALID_ARG, "%s: need 1 <= sx, sy, sz <= 4096 and sx * sy * sz <= 2^30 (got %d, %d, %d)", fn, sx,
                    sy, sz);
    if (int rc = check_int_range(fn, "x0", x0, -8192, 8192)) return rc;
    if (int rc = check_int_range(fn, "y0", y0, -8192, 8192)) return rc;
    if (int rc = check_int_range(fn, "z0", z0, -8192, 8192)) return rc;
    if (rx < 0 || ry < 0 || rz < 0 || cx < 1 || cy < 1 || cz < 1 || rx > sx - cx || ry > sy - cy || rz > sz - cz)
        return fail(SMX_ERR_INVALID_ARG,
                    "%s: the region must lie inside the source: need rx, ry, rz >= 0, cx, cy, cz >= 1 and rx + cx <= sx, "
                    "ry + cy <= sy, rz + cz <= sz (got start %d, %d, %d and dims %d, %d, %d in %d, %d, %d)", fn, rx, ry, rz,
                    cx, cy, cz, sx, sy, sz);
    if (int rc = check_int_range(fn, "mode", mode, SMX_TSDF_MERGE_FILL, SMX_TSDF_MERGE_AVERAGE)) return rc;
    if (int rc = check_positive(fn, "max_weight", max_weight)) return rc;
    const size_t vox = (size_t)nx * ny * nz, svox = (size_t)sx * sy * sz;
    if (int rc = check_disjoint(fn, {{src_tsdf, svox * sizeof(float)}, {src_weight, svox * sizeof(float)}, {src_color, svox * 4}},
                                {{tsdf, vox * sizeof(float)}, {weight, vox * sizeof(float)}, {color, vox * 4}},
                                "a destination array overlaps a source array (a volume cannot be merged into itself)",
                                "two destination arrays overlap"))
        return rc;
    if (int rc = check_caller_stream(fn, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_tsdf_merge(nx, ny, nz, tsdf, weight, color, sx, sy, sz, src_tsdf, src_weight, src_color, x0, y0, z0, rx,
                               ry, rz, cx, cy, cz, mode, max_weight, (hipStream_t)stream);
    });
}

// ---- camera tracking ---------------------------------------------------------------------------------------------------
static bool track_dims_ok(int n, int H, int W) {
    return points_dims_ok(n, H, W) && track_grid(H, W, 1).tiles <= TRK_MAX_TILES;
}

size_t smx_track_camera_workspace_bytes(int n, int H, int W) {
    return track_dims_ok(n, H, W) ? track_layout(n, H, W).total : 0;
}

// The checks smx_track_camera, smx_track_camera_photometric and smx_track_camera_pyramid share, in their order: everything
// before the workspace's size.  photo: the photometric entries' term, whose two planes (named `planes`: the pyramid entry's
// are its pyramids) are part of the NULL check.
static int check_track_args(const char *fn, const smx::TrackCall &c, const smx::TrackPhotoTerm *photo, const char *planes) {
    const int n = c.n, H = c.H, W = c.W, Hm = c.Hm, Wm = c.Wm, schedule_pairs = c.pairs;
    const float *Q = c.q, *Qm = c.qm, *Pm = c.pm;
    const int32_t *schedule = c.schedule;
    if (photo && (!photo->frame_intensity || !photo->model_intensity))
        return fail(SMX_ERR_INVALID_ARG, "%s: frame_%s and model_%s must be non-NULL", fn, planes, planes);
    if (!c.disp || !Q || !c.model_depth || !c.model_normals || !Qm || !Pm || !c.model_camera_to_world ||
        !c.model_world_to_camera || !c.pose_in || !c.pose_out || !c.workspace)
        return fail(SMX_ERR_INVALID_ARG,
                    "%s: disp, Q, model_depth, model_normals, Qm, Pm, model_camera_to_world, model_world_to_camera, "
                    "pose_in, pose_out and workspace must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_pixel_count(fn, n, H, W)) return rc;
    if (track_grid(H, W, 1).tiles > TRK_MAX_TILES)
        return fail(SMX_ERR_INVALID_ARG, "%s: ceil(W / %d) * ceil(H / %d) = %d tiles exceed the limit of %d", fn, TRK_COLS,
                    TRK_ROWS, track_grid(H, W, 1).tiles, TRK_MAX_TILES);
    if (!map_dims_ok(n, Hm, Wm) || (long)n * Hm * Wm > SMX_POINTS_MAX)
        return fail(SMX_ERR_INVALID_ARG, "%s: need 1 <= Hm, Wm <= 32768 and n * Hm * Wm <= 2^30 (got Hm %d, Wm %d)", fn, Hm,
                    Wm);
    for (int k = 0; k < 16; ++k) {                            // one loop: the lower index is reported, Q, Qm, then Pm
        if (int rc = check_finite_at(fn, "Q", Q, k)) return rc;
        if (int rc = check_finite_at(fn, "Qm", Qm, k)) return rc;
        if (int rc = check_finite_at(fn, "Pm", Pm, k)) return rc;
    }
    if (Qm[2] != 0.0f || Qm[6] != 0.0f || Qm[10] != 0.0f || Qm[12] != 0.0f || Qm[13] != 0.0f || Qm[14] == 0.0f)
        return fail(SMX_ERR_INVALID_ARG,
                    "%s: Qm's ray must not depend on d: need Qm02 = Qm12 = Qm22 = 0, Qm30 = Qm31 = 0 and Qm32 != 0", fn);
    if (int rc = check_reprojection_args(fn, c.zmin, c.zmax, c.min_confidence, c.invalid, nullptr, 0, 0, nullptr, ""))
        return rc;
    if (int rc = check_int_range(fn, "schedule_pairs", schedule_pairs, 0, 8)) return rc;
    if (schedule_pairs > 0 && !schedule) return fail(SMX_ERR_INVALID_ARG, "%s: schedule must be non-NULL", fn);
    int iterations = 0;
    for (int p = 0; p < schedule_pairs; ++p) {
        if (int rc = check_int_range(fn, "a schedule stride", schedule[2 * p], 1, 32768)) return rc;
        if (int rc = check_int_range(fn, "a schedule iteration count", schedule[2 * p + 1], 0, 64)) return rc;
        iterations += schedule[2 * p + 1];
    }
    if (int rc = check_int_range(fn, "the schedule's iterations in total", iterations, 0, 64)) return rc;
    if (int rc = check_positive(fn, "max_distance", c.max_distance)) return rc;
    if (int rc = check_int_range(fn, "min_inliers", c.min_inliers, 1, 1 << 30)) return rc;
    if (int rc = check_non_negative(fn, "min_pivot", c.min_pivot)) return rc;
    if (int rc = check_non_negative(fn, "rot_eps", c.rot_eps)) return rc;
    if (int rc = check_non_negative(fn, "trans_eps", c.trans_eps)) return rc;
    return SMX_OK;
}

// The rules of smx_track_camera_pyramid's own arguments, after check_track_args has passed the schedule.
static int check_track_pyramid_args(const char *fn, const smx::TrackCall &c, const smx::TrackPyramidTerm &t) {
    if (int rc = check_int_range(fn, "levels", t.levels, 1, PYR_MAX_LEVELS)) return rc;
    if (c.pairs > 0 && !t.schedule_levels) return fail(SMX_ERR_INVALID_ARG, "%s: schedule_levels must be non-NULL", fn);
    for (int p = 0; p < c.pairs; ++p) {
        const int level = t.schedule_levels[p], stride = c.schedule[2 * p];
        if (int rc = check_int_range(fn, "a schedule level", level, 0, t.levels - 1)) return rc;
        if (stride % (1 << level) != 0)
            return fail(SMX_ERR_INVALID_ARG, "%s: a stride must be divisible by 2^level (got stride %d at level %d)", fn, stride,
                        level);
    }
    if (!(t.huber_delta > 0.0f))                                    // +inf passes: no robust weights
        return fail(SMX_ERR_INVALID_ARG, "%s: huber_delta must be > 0, got %g", fn, (double)t.huber_delta);
    return SMX_OK;
}

// smx_track_camera, smx_track_camera_photometric and smx_track_camera_pyramid: photo NULL is smx_track_camera; with pyr,
// photo holds the term's arguments that the two photometric entries share and the pyramids in place of the planes.
static int track_entry(const char *fn, int device_id, const smx::TrackCall &c, const smx::TrackPhotoTerm *photo,
                       const smx::TrackPyramidTerm *pyr, size_t workspace_bytes, void *stream) {
    if (int rc = check_track_args(fn, c, photo, pyr ? "pyramid" : "intensity")) return rc;
    if (photo) {
        if (int rc = check_non_negative(fn, "photometric_weight", photo->weight)) return rc;
        if (int rc = check_positive(fn, "max_intensity_difference", photo->max_intensity_difference)) return rc;
    }
    if (pyr)
        if (int rc = check_track_pyramid_args(fn, c, *pyr)) return rc;
    if (int rc = photo ? check_workspace_bytes(fn, "smx_track_camera_photometric_workspace_bytes", workspace_bytes,
                                               track_photo_layout(c.n, c.H, c.W).total)
                       : check_workspace_bytes(fn, "smx_track_camera_workspace_bytes", workspace_bytes,
                                               track_layout(c.n, c.H, c.W).total))
        return rc;
    const size_t n = (size_t)c.n, map_bytes = n * c.H * c.W * sizeof(float), model_bytes = n * c.Hm * c.Wm * sizeof(float);
    const size_t pose_bytes = n * 12 * sizeof(float);
    const size_t frame_bytes = pyr ? pyramid_level(c.n, c.H, c.W, pyr->levels).offset * sizeof(float) : map_bytes;
    const size_t view_bytes = pyr ? pyramid_level(c.n, c.Hm, c.Wm, pyr->levels).offset * sizeof(float) : model_bytes;
    const smx::TrackPhotoTerm none{}, &t = photo ? *photo : none;    // a NULL span overlaps nothing
    if (int rc = check_disjoint(fn, {{c.disp, map_bytes}, {c.confidence, map_bytes}, {c.model_depth, model_bytes},
                                     {c.model_normals, 3 * model_bytes}, {c.model_camera_to_world, pose_bytes},
                                     {c.model_world_to_camera, pose_bytes},
                                     {c.pose_in != c.pose_out ? c.pose_in : nullptr, pose_bytes},
                                     {t.frame_intensity, frame_bytes}, {t.model_intensity, view_bytes}},
                                {{c.pose_out, pose_bytes}, {c.info, n * 4 * sizeof(int32_t)}, {c.rms, n * sizeof(float)},
                                 {c.normal_equations, n * (photo ? TRKP_TERMS : TRK_TERMS) * sizeof(double)},
                                 {t.info, n * 2 * sizeof(int32_t)}, {t.rms, n * sizeof(float)},
                                 {c.workspace, workspace_bytes}},
                                "an output or the workspace overlaps an input (pose_out may be pose_in itself)",
                                "two outputs (the workspace is one) overlap"))
        return rc;
    if (int rc = check_workspace_and_stream(fn, c.workspace, stream)) return rc;
    return launch_on(device_id, [&] {
        if (pyr) smx::launch_track_camera_pyramid(c, *photo, *pyr, (hipStream_t)stream);
        else if (photo) smx::launch_track_camera_photometric(c, *photo, (hipStream_t)stream);
        else smx::launch_track_camera(c, (hipStream_t)stream);
    });
}

int smx_track_camera(int device_id, int n, int H, int W, const float *disp, const float *confidence, const float Q[16],
                     float min_confidence, float z_min, float z_max, float invalid_disparity, int Hm, int Wm,
                     const float *model_depth, const float *model_normals, const float Qm[16], const float Pm[16],
                     const float *model_camera_to_world, const float *model_world_to_camera, const float *pose_in,
                     int schedule_pairs, const int32_t *schedule, float max_distance, int min_inliers, float min_pivot,
                     float rot_eps, float trans_eps, float *pose_out, int32_t *info, float *rms,
                     double *normal_equations, void *workspace, size_t workspace_bytes, void *stream) {
    const smx::TrackCall c{n, H, W, disp, confidence, Q, min_confidence, z_min, z_max, invalid_disparity, Hm, Wm,
                           model_depth, model_normals, Qm, Pm, model_camera_to_world, model_world_to_camera, pose_in,
                           schedule_pairs, schedule, max_distance, min_inliers, min_pivot, rot_eps, trans_eps, pose_out,
                           info, rms, normal_equations, workspace};
    return track_entry("smx_track_camera", device_id, c, nullptr, nullptr, workspace_bytes, stream);
}

size_t smx_track_camera_photometric_workspace_bytes(int n, int H, int W) {
    return track_dims_ok(n, H, W) ? track_photo_layout(n, H, W).total : 0;
}

int smx_track_camera_photometric(int device_id, int n, int H, int W, const float *disp, const float *confidence,
                                 const float Q[16], float min_confidence, float z_min, float z_max,
                                 float invalid_disparity, int Hm, int Wm, const float *model_depth,
                                 const float *model_normals, const float Qm[16], const float Pm[16],
                                 const float *model_camera_to_world, const float *model_world_to_camera,
                                 const float *pose_in, int schedule_pairs, const int32_t *schedule, float max_distance,
                                 int min_inliers, float min_pivot, float rot_eps, float trans_eps,
                                 const float *frame_intensity, const float *model_intensity, float photometric_weight,
                                 float max_intensity_difference, float *pose_out, int32_t *info, float *rms,
                                 double *normal_equations, int32_t *photometric_info, float *photometric_rms,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    const smx::TrackCall c{n, H, W, disp, confidence, Q, min_confidence, z_min, z_max, invalid_disparity, Hm, Wm,
                           model_depth, model_normals, Qm, Pm, model_camera_to_world, model_world_to_camera, pose_in,
                           schedule_pairs, schedule, max_distance, min_inliers, min_pivot, rot_eps, trans_eps, pose_out,
                           info, rms, normal_equations, workspace};
    const smx::TrackPhotoTerm photo{frame_intensity, model_intensity, photometric_weight, max_intensity_difference,
                                    photometric_info, photometric_rms};
    return track_entry("smx_track_camera_photometric", device_id, c, &photo, nullptr, workspace_bytes, stream);
}

int smx_track_camera_pyramid(int device_id, int n, int H, int W, const float *disp, const float *confidence,
                             const float Q[16], float min_confidence, float z_min, float z_max, float invalid_disparity,
                             int Hm, int Wm, const float *model_depth, const float *model_normals, const float Qm[16],
                             const float Pm[16], const float *model_camera_to_world, const float *model_world_to_camera,
                             const float *pose_in, int schedule_pairs, const int32_t *schedule, float max_distance,
                             int min_inliers, float min_pivot, float rot_eps, float trans_eps, const float *frame_pyramid,
                             const float *model_pyramid, int levels, const int32_t *schedule_levels,
                             float photometric_weight, float max_intensity_difference, float huber_delta, float *pose_out,
                             int32_t *info, float *rms, double *normal_equations, int32_t *photometric_info,
                             float *photometric_rms, void *workspace, size_t workspace_bytes, void *stream) {
    const smx::TrackCall c{n, H, W, disp, confidence, Q, min_confidence, z_min, z_max, invalid_disparity, Hm, Wm,
                           model_depth, model_normals, Qm, Pm, model_camera_to_world, model_world_to_camera, pose_in,
                           schedule_pairs, schedule, max_distance, min_inliers, min_pivot, rot_eps, trans_eps, pose_out,
                           info, rms, normal_equations, workspace};
    const smx::TrackPhotoTerm photo{frame_pyramid, model_pyramid, photometric_weight, max_intensity_difference,
                                    photometric_info, photometric_rms};
    const smx::TrackPyramidTerm pyr{levels, schedule_levels, huber_delta};
    return track_entry("smx_track_camera_pyramid", device_id, c, &photo, &pyr, workspace_bytes, stream);
}

int smx_intensity_planes(int device_id, int n, int channels, int H, int W, const uint8_t *image, float *out,
                         void *stream) {
    const char *fn = "smx_intensity_planes";
    if (!image || !out) return fail(SMX_ERR_INVALID_ARG, "%s: image and out must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_pixel_count(fn, n, H, W)) return rc;
    if (channels != 1 && channels != 3)
        return fail(SMX_ERR_INVALID_ARG, "%s: channels must be 1 or 3, got %d", fn, channels);
    const size_t px = (size_t)n * H * W;
    if (int rc = check_disjoint(fn, {{image, px * channels}}, {{out, px * sizeof(float)}}, "out must not overlap image"))
        return rc;
    if (int rc = check_caller_stream(fn, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_intensity_planes(n, channels, H, W, image, out, (hipStream_t)stream);
    });
}

size_t smx_intensity_pyramid_bytes(int n, int H, int W, int levels) {
    if (!points_dims_ok(n, H, W) || levels < 1 || levels > PYR_MAX_LEVELS) return 0;
    return pyramid_level(n, H, W, levels).offset * sizeof(float);
}

int smx_intensity_pyramid(int device_id, int n, int H, int W, int levels, const float *plane, const float *mask_depth,
                          float *pyramid, void *stream) {
    const char *fn = "smx_intensity_pyramid";
    if (!plane || !pyramid) return fail(SMX_ERR_INVALID_ARG, "%s: plane and pyramid must be non-NULL", fn);
    if (int rc = check_map_dims(fn, n, H, W)) return rc;
    if (int rc = check_pixel_count(fn, n, H, W)) return rc;
    if (int rc = check_int_range(fn, "levels", levels, 1, PYR_MAX_LEVELS)) return rc;
    const size_t px = (size_t)n * H * W;
    if (int rc = check_disjoint(fn, {{plane, px * sizeof(float)}, {mask_depth, px * sizeof(float)}},
                                {{pyramid, smx_intensity_pyramid_bytes(n, H, W, levels)}},
                                "pyramid must not overlap plane or mask_depth"))
        return rc;
    if (int rc = check_caller_stream(fn, stream)) return rc;
    return launch_on(device_id, [&] {
        smx::launch_intensity_pyramid(n, H, W, levels, plane, mask_depth, pyramid, (hipStream_t)stream);
    });
}

}  // extern "C"
