// smx_launch.h -- host-side launch interface between the C ABI (smx_engine.hip, smx_maps.hip) and the kernel
// translation units (tu_*.hip).  Every kernel family is compiled in its own translation unit so that the
// library builds in parallel and a change to one kernel recompiles one file; the C ABI's units never instantiate
// a kernel template themselves.  All functions enqueue on `s` and return without synchronising.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "smx_common.h"

namespace smx {

struct RefineParams;      // k_refine.h
struct FillParams;        // k_fill.h
struct FilterParams;      // k_match_filter.h

// ---- tu_stages.hip: steps 1-2, 6, 7-9 and the "next"-row kernels ------------------------------------------
struct PrologueArgs {
    const void *left, *right;
    float *gray_l, *gray_r, *down_l, *down_r;
    int *flags, *flags2;
    uint8_t *g8_l, *g8_r;
    uint16_t *units_l, *units_r;      // [n][h][upitch] the pooled planes in grid units (smx_common.h: MatchParams::Lu)
    int H, W, K, h, w, grid_capable, pitch8, padl, padr, epoch, gpitch, gpadl, upitch;
    int fp_conv;             // smx_fp_convention (RGB entries: step 1)
};
// like the aggregation family below, these three are tables from their launch spec (smx_common.h) to an instantiation
void launch_prologue(const PrologueLaunch &x, const PrologueArgs &a, int n, hipStream_t s);
void launch_refine(const RefineLaunch &x, const RefineParams &p, int n, hipStream_t s);
void launch_fill(const FillLaunch &x, const FillParams &p, int n, hipStream_t s);
void launch_flag_to_bool(const int *flag, int epoch, int *out, hipStream_t s);
void launch_metrics(int n, const float *est, const float *gt, const uint8_t *mask, size_t pixels, float max_disparity,
                    const float thresholds[4], double *out_sums, hipStream_t s);
void launch_points(const float *disp, int H, int W, float bf, float invalid, float *depth, float *points, int *count_dev,
                   int *workspace, hipStream_t s);

// ---- the aggregation family: every launcher is a table from its launch spec (smx_common.h; filled by plan_range,
// smx_plan.h) to a kernel instantiation and decides nothing itself
// ---- tu_exact.hip: the exact-order aggregation kernels ----------------------------------------------------
void launch_exact(const ExactLaunch &x, const MatchParams &p, int n, hipStream_t s);
void launch_exact2_capture(const ExactCaptureLaunch &x, const MatchParams &p, int n, hipStream_t s);
// p.nd_chunk: the engine's exact2_nd; stats_dev / stats_host: candidate density of the launch, published to pinned host
// memory (k_match_exact2.h: SparseStats); may be NULL
void launch_exact2_sparse(const MatchParams &p, int n, unsigned *cand, int cw, const int *range_flags, unsigned *stats_dev,
                          unsigned long long *stats_host, unsigned seq, hipStream_t s);
hipError_t exact_raise_lds_caps(int cap_bytes);

// ---- tu_fast_*.hip: the running-sum (FAST_GRID) aggregation kernels ---------------------------------------
void launch_match_fast(const FastLaunch &fl, const MatchParams &p, int n, hipStream_t s);
void launch_match_fast_tall_24(const FastLaunch &fl, const MatchParams &p, int n, hipStream_t s);
void launch_match_fast_tall_27(const FastLaunch &fl, const MatchParams &p, int n, hipStream_t s);
void launch_match_fast_tall_32(const FastLaunch &fl, const MatchParams &p, int n, hipStream_t s);
void launch_match_fast_stack(const FastLaunch &fl, const MatchParams &p, int n, hipStream_t s);     // tu_fast_stack.hip: fl.stack == 2
hipError_t fast_stack_raise_caps();       // ... whose tile needs more than 64 KB of LDS
void launch_match_auto_small_tu(const AutoLaunch &al, const MatchParams &p, int n, hipStream_t s);
hipError_t match_auto_raise_caps();       // k_match_auto.h: MATCH_AUTO_LDS_CAP

// ---- tu_capture.hip: min_disparity > 0 without the volume -------------------------------------------------
void launch_match_capture_tu(const FastCaptureLaunch &cl, const MatchParams &p, int n, hipStream_t s);

// ---- tu_filter_*.hip: candidate marking of the filtered exact-order route ---------------------------------
void launch_match_filter_tu(const FilterLaunch &fl, const MatchParams &p, const FilterParams &f, int n, hipStream_t s);
void launch_match_filter_24(const FilterLaunch &fl, const MatchParams &p, const FilterParams &f, int n, hipStream_t s);
void launch_match_filter_27(const FilterLaunch &fl, const MatchParams &p, const FilterParams &f, int n, hipStream_t s);
void launch_match_filter_32(const FilterLaunch &fl, const MatchParams &p, const FilterParams &f, int n, hipStream_t s);

// ---- tu_lr.hip: left-right consistency check (k_lr.h) ----------------------------------------------------
// rows = n * planes * H rows of W elements of elem_bytes (1 or 4) per input; pl / pr: [2n] pairs, the second n mirrored
void launch_lr_pack(int elem_bytes, const void *l, const void *r, void *pl, void *pr, long rows, int W, hipStream_t s);
// mirrored: `right` holds the raw output of the mirrored internal pairs (flip(D_R)); right_out may be NULL
void launch_lr_check(bool mirrored, const float *left, const float *right, float *out, float *right_out, int n, int H, int W,
                     float max_diff, float invalid, hipStream_t s);

// ---- tu_post.hip: speckle filter and hole fill (k_post.h) --------------------------------------------------------
// workspace: smx_workspace.h: post_layout(n, H, W)
void launch_filter_speckles(int n, int H, int W, const float *in, float *out, int max_size, float max_diff, float invalid,
                            void *workspace, hipStream_t s);
void launch_fill_invalid(int n, int H, int W, const float *in, float *out, float invalid, void *workspace, hipStream_t s);

// ---- tu_median.hip: image-guided weighted median (k_median.h) ------------------------------------------------------
// range / spatial: the host tables, copied into the kernel arguments (spatial holds (radius+1)^2 entries)
size_t median_workspace_bytes(int n, int H, int W);
void launch_weighted_median(int n, int H, int W, const float *in, const float *holes, const float *guide, float *out,
                            int radius, const uint16_t *range, const uint16_t *spatial, float invalid, hipStream_t s);

// ---- tu_wls.hip: image-guided weighted least squares filter (k_wls.h) ----------------------------------------------
// workspace: smx_workspace.h: wls_layout(n, H, W); lambdas[iterations] and range[256]: the host tables, copied into the
// kernel arguments; arguments checked by smx_wls_filter
void launch_wls(int n, int H, int W, const float *in, const float *conf, const float *guide, float *out, int iterations,
                const float *lambdas, const float *range, float min_weight, float invalid, void *workspace,
                hipStream_t s);

// ---- tu_confidence.hip: per-pixel confidence (k_confidence.h) -----------------------------------------------------
// right / guide NULL: no LR / texture term; arguments checked by smx_confidence_map
void launch_confidence(int n, int H, int W, const float *left, const float *right, const float *guide, int radius,
                       float lr_scale, float texture_scale, float invalid, float *out, hipStream_t s);

// ---- tu_temporal.hip: motion-gated temporal filter (k_temporal.h) ---------------------------------------------------
// conf / guide_out NULL: every valid measurement weighs 1 / no copy of the guide; arguments checked by
// smx_temporal_filter
void launch_temporal(int n, int H, int W, const float *disp, const float *conf, const float *guide,
                     const float *prev_guide, float *state_disp, float *state_weight, float *guide_out, float *out,
                     int radius, float threshold, float decay, float max_diff, float max_weight, float min_weight,
                     float invalid, hipStream_t s);

// ---- tu_remap.hip: bilinear remap / rectification (k_remap.h) -------------------------------------------------------
// in_r / map_r / out_r NULL: left view only; arguments checked by smx_remap_pairs
void launch_remap_pairs(int n, int C, bool f32, int Hi, int Wi, int Ho, int Wo, const void *in_l, const void *in_r,
                        const int32_t *map_l, const int32_t *map_r, void *out_l, void *out_r, bool replicate,
                        float border_value, hipStream_t s);

// ---- tu_synthesis.hip: right-view synthesis head (k_synthesis.h) ------------------------------------------------------
// left / out: [n][C][h*S][w*S], C 1 or 3; arguments checked by smx_synthesize_right_view
void launch_synthesis(int n, int C, bool f32, int D, int h, int w, int S, const float *prob, const void *left, float *out,
                      hipStream_t s);
// the training form: the sums themselves, without the rescale; arguments checked by smx_synthesis_head_forward
void launch_synthesis_view(int n, int C, bool f32, int D, int h, int w, int S, const float *prob, const void *left,
                           float *view, hipStream_t s);

// ---- tu_synthesis_grad.hip: backward of the synthesis head (k_synthesis_grad.h) --------------------------------------
// grad_view / left: [n][C][h*S][w*S]; grad_prob: [n][D][h][w]; arguments checked by smx_synthesis_head_backward
void launch_synthesis_grad(int n, int C, bool f32, int D, int h, int w, int S, const float *grad_view, const void *left,
                           float *grad_prob, hipStream_t s);

// ---- tu_sgm.hip: semi-global matching (k_sgm.h) ----------------------------------------------------------------------
// workspace: smx_workspace.h: sgm_layout(n, H, W, D); right_out NULL: not written (the
// right-view WTA runs only for the LR check); arguments checked by smx_sgm / smx_sgm_with_right_map
void launch_sgm(int n, int C, bool f32, int H, int W, const void *left, const void *right, int dmin, int D, int paths,
                int P1, int P2, int uniqueness, float lr_max_diff, bool subpixel, float invalid, float *out,
                float *gray_out, float *right_out, void *workspace, hipStream_t s);

// ---- tu_reproject.hip: metric 3D points and voxel-grid downsampling (k_reproject.h) ------------------------------------
// q: the host's 4x4 matrix, copied into the kernel arguments; conf / image / colors / indices / xyz_map may be NULL;
// workspace: reproject_layout(n, H); arguments checked by smx_reproject_points
void launch_reproject(int n, int H, int W, const float *disp, const float q[16], const float *conf, float min_conf,
                      float zmin, float zmax, float invalid, const void *image, int channels, bool img_f32,
                      float *points, uint8_t *colors, int32_t *indices, float *xyz_map, int32_t *offsets,
                      void *workspace, hipStream_t s);
// colors / out_colors NULL: no colour; workspace: vox_layout(n, capacity); arguments checked by smx_voxel_downsample
hipError_t launch_voxel_downsample(int n, int capacity, const float *points, const uint8_t *colors,
                                   const int32_t *offsets, float voxel_size, int min_points, float *out_points,
                                   uint8_t *out_colors, int32_t *out_counts, int32_t *out_offsets, int32_t *dropped,
                                   void *workspace, hipStream_t s);
// exclusive scan of L ints, in -> out, in three launches; block_sums: scan_block_sums(L) ints (smx_workspace.h); gate / pass:
// a launch returns at once when gate != NULL and pass * 8 >= *gate (the radix passes of the downsampling)
void launch_scan(const int *in, int *out, long L, int *block_sums, const int *gate, int pass, hipStream_t s);

// ---- tu_project.hip: point clouds projected into camera views with a depth test (k_project.h) ---------------------------
// p: the host's 4x4 matrix, copied into the kernel arguments; index / depth may be NULL; workspace:
// project_layout(n, H, W); arguments checked by smx_project_points
void launch_project(int n, int capacity, int H, int W, const float *points, const int32_t *offsets,
                    const float *world_to_camera, const float p[16], int radius, float zmin, float zmax, float invalid,
                    float *disp, int32_t *index, float *depth, void *workspace, hipStream_t s);

// ---- tu_tsdf.hip: TSDF fusion and surface extraction (k_tsdf.h, k_mesh.h) --------------------------------------------------------
// q / p / origin: host values, copied into the kernel arguments; world_to_camera [n][3][4] on the device; conf / color /
// image may be NULL (color needs image); workspace: tsdf_integrate_layout(n, H, W); arguments checked by smx_tsdf_integrate
void launch_tsdf_integrate(int nx, int ny, int nz, const float origin[3], float voxel_size, float truncation,
                           float max_weight, float *tsdf, float *weight, uint8_t *color, int n, int H, int W,
                           const float *disp, const float q[16], const float p[16], const float *world_to_camera,
                           const float *conf, float min_conf, float zmin, float zmax, float invalid, const void *image,
                           int channels, bool img_f32, void *workspace, hipStream_t s);
// normals / colors NULL: not written (colors needs color); workspace: tsdf_extract_layout(ny, nz); checked by smx_tsdf_extract_points
void launch_tsdf_extract(int nx, int ny, int nz, const float origin[3], float voxel_size, const float *tsdf,
                         const float *weight, const uint8_t *color, float min_weight, int capacity, float *points,
                         float *normals, uint8_t *colors, int32_t *count, void *workspace, hipStream_t s);
// the triangles over those points (k_mesh.h); workspace: mesh_layout(nx, ny, nz); checked by smx_tsdf_extract_triangles
void launch_tsdf_triangles(int nx, int ny, int nz, const float *tsdf, const float *weight, float min_weight,
                           int capacity, int32_t *triangles, int32_t *count, void *workspace, hipStream_t s);

// ---- tu_raycast.hip: views of a TSDF volume by ray casting (k_raycast.h) -------------------------------------------------
// q / origin: host values, copied into the kernel arguments; camera_to_world [n][3][4] on the device; M: the number of
// samples per ray; color / depth / normals / colors / out_weight may be NULL (colors needs color); workspace:
// raycast_layout(nx, ny, nz); arguments checked by smx_tsdf_raycast
void launch_tsdf_raycast(int nx, int ny, int nz, const float origin[3], float voxel_size, const float *tsdf,
                         const float *weight, const uint8_t *color, float min_weight, int n, int H, int W,
                         const float q[16], const float *camera_to_world, float step, float zmin, int M, float invalid,
                         float *disp, float *depth, float *normals, uint8_t *colors, float *out_weight, void *workspace,
                         hipStream_t s);

// ---- tu_tsdf_window.hip: a window of a volume's state as a volume of its own (k_tsdf_window.h) ---------------------------
// color and color_out both NULL or both given; one launch, no workspace; arguments checked by smx_tsdf_window
void launch_tsdf_window(int nx, int ny, int nz, const float *tsdf, const float *weight, const uint8_t *color, int x0,
                        int y0, int z0, int bx, int by, int bz, float *tsdf_out, float *weight_out, uint8_t *color_out,
                        hipStream_t s);

// ---- tu_tsdf_merge.hip: one volume's state merged into another in place (k_tsdf_merge.h) -------------------------------
// color and src_color both NULL or both given; one launch (none if the region misses the destination), no workspace;
// arguments checked by smx_tsdf_merge
void launch_tsdf_merge(int nx, int ny, int nz, float *tsdf, float *weight, uint8_t *color, int sx, int sy, int sz,
                       const float *src_tsdf, const float *src_weight, const uint8_t *src_color, int x0, int y0, int z0,
                       int rx, int ry, int rz, int cx, int cy, int cz, int mode, float max_weight, hipStream_t s);

// ---- tu_track.hip, tu_track_photo.hip: camera tracking against rendered model views (k_track.h, k_track_photo.h) ----------
// A call's operands in the C entries' order.  q / qm / pm / schedule ([pairs][2]: stride, iterations): host values; every
// other pointer is device memory; confidence, info, rms and normal_equations ([n][30], with the photometric term
// [n][33]) may be NULL; arguments checked by smx_track_camera, smx_track_camera_photometric and smx_track_camera_pyramid
struct TrackCall {
    int n, H, W;
    const float *disp, *confidence, *q;
    float min_confidence, zmin, zmax, invalid;
    int Hm, Wm;
    const float *model_depth, *model_normals, *qm, *pm, *model_camera_to_world, *model_world_to_camera, *pose_in;
    int pairs;
    const int32_t *schedule;
    float max_distance;
    int min_inliers;
    float min_pivot, rot_eps, trans_eps;
    float *pose_out;
    int32_t *info;
    float *rms;
    double *normal_equations;
    void *workspace;
};
// the photometric term: the two intensity planes (device), its weight and threshold, and its outputs, which may be NULL
struct TrackPhotoTerm {
    const float *frame_intensity, *model_intensity;
    float weight, max_intensity_difference;
    int32_t *info;
    float *rms;
};
// workspace: track_layout(n, H, W)
void launch_track_camera(const TrackCall &c, hipStream_t s);
// workspace: track_photo_layout(n, H, W)
void launch_track_camera_photometric(const TrackCall &c, const TrackPhotoTerm &t, hipStream_t s);
// in: uint8 [n][C][H][W], C 1 or 3; out: f32 [n][H][W]; arguments checked by smx_intensity_planes
void launch_intensity_planes(int n, int C, int H, int W, const uint8_t *in, float *out, hipStream_t s);

// ---- tu_pyramid.hip, tu_track_pyramid.hip: intensity pyramids, and tracking that reads them (k_pyramid.h, k_track_pyramid.h) ----
// plane, mask_depth (may be NULL): [n][H][W]; pyramid: the levels one after another, level l [n][H_l][W_l] with
// H_l = ceil(H / 2^l) (smx_workspace.h: pyramid_level); one launch per level, no workspace; arguments checked by
// smx_intensity_pyramid
void launch_intensity_pyramid(int n, int H, int W, int levels, const float *plane, const float *mask_depth, float *pyramid,
                              hipStream_t s);
// what the photometric term takes on when it is read from pyramids: TrackPhotoTerm's two planes are then pyramids
// (device) of `levels` levels; the level of every schedule pair (host), and Huber's bound
struct TrackPyramidTerm {
    int levels;
    const int32_t *schedule_levels;
    float huber_delta;
};
// workspace: track_photo_layout(n, H, W)
void launch_track_camera_pyramid(const TrackCall &c, const TrackPhotoTerm &t, const TrackPyramidTerm &py, hipStream_t s);

}  // namespace smx
