/*
 * stereo_mi355x.h -- C ABI of libstereo_mi355x.so, the MI355X-native (gfx950, hand-written
 * HIP) replacement for the reference's "CUDA stereo matching" engine.
 *
 * This is the drop-in boundary.  The reference exposes the path as a pybind11 torch
 * extension (`cuda_depth`, /root/reference/src/csrc/depth/torch_extension_module.cc:6-27);
 * the entry points below are what a ctypes / cgo / JNI binding of that same surface binds
 * to.  No torch / C++ types cross the boundary: plain structs, device pointers, sizes.
 *
 *   reference interface                                   replaced by
 *   ----------------------------------------------------  --------------------------------
 *   struct stereo_matching_configuration                  smx_config (first 11 fields, same
 *     depth/stereo_matching_configuration.hh:5-17           order, same defaults)
 *   stereo_matching::stereo_matching(config)              smx_create
 *     depth/stereo_matching.cc:17-20 + device_buffer
 *     depth/buffer/device_buffer.cc:3-12 (8 buffers)
 *   stereo_matching::compute_disparity_map(left,right)    smx_compute_rgb  ([3][H][W] f32, as the
 *     depth/stereo_matching.cc:22-43                        reference's callers pass it)
 *   -- (grayscale entry, skips step 1; BASELINE configs)  smx_compute_gray / smx_compute_gray_u8
 *   -- (independent pairs, one launch set)                smx_compute_gray_batch / _rgb_batch
 *                                                         / _gray_u8_batch / _rgb_u8_batch
 *   -- (left-right consistency check)                     smx_compute_lr_*_batch, smx_lr_check
 *   -- (speckle filter, hole fill)                        smx_filter_speckles, smx_fill_invalid
 *   -- (image-guided weighted median)                     smx_weighted_median
 *   -- (image-guided weighted least squares filter)       smx_wls_filter, smx_wls_workspace_bytes
 *   -- (per-pixel confidence: LR agreement x texture)     smx_confidence_map
 *   -- (motion-gated temporal filter of map streams)      smx_temporal_filter
 *   -- (rectification of raw frames: bilinear remap)      smx_remap_pairs
 *   Deep3D's selection layer, upsampling and rescale      smx_synthesize_right_view (the head only: the
 *     python/pipeline/synthesis/deep3d.py:155,162-183,      network is the caller's)
 *     synthesis/kernels/rescale_generated_view.cu
 *   the same layer inside the reference's training loop   smx_synthesis_head_forward, smx_synthesis_head_backward
 *     python/pipeline/synthesis/trainer.py (autograd)       (the view in 0..1 and the volume's gradient)
 *   -- (semi-global matching, census cost: 2nd matcher)   smx_sgm, smx_sgm_workspace_bytes,
 *                                                         smx_sgm_with_right_map
 *   -- (metric 3D points, coloured, compacted)            smx_reproject_points, smx_reproject_workspace_bytes
 *   -- (voxel-grid downsampling of those points)          smx_voxel_downsample, smx_voxel_workspace_bytes
 *   -- (those points back into a camera: z-buffered map)  smx_project_points, smx_project_workspace_bytes
 *   -- (TSDF fusion of posed maps into a voxel volume)    smx_tsdf_integrate, smx_tsdf_integrate_workspace_bytes
 *   -- (surface points of that volume, ordered)           smx_tsdf_extract_points, smx_tsdf_extract_workspace_bytes
 *   -- (triangles over those points: marching cubes)      smx_tsdf_extract_triangles,
 *                                                         smx_tsdf_extract_triangles_workspace_bytes
 *   -- (disparity, normal and colour views of that volume) smx_tsdf_raycast, smx_tsdf_raycast_workspace_bytes
 *   -- (a window of that volume: shift, crop, grow, spill) smx_tsdf_window
 *   -- (one volume's state merged into another: restore, join) smx_tsdf_merge
 *   -- (the camera pose of a frame against such a view)   smx_track_camera, smx_track_camera_workspace_bytes
 *   -- (the same with a photometric term; its planes)     smx_track_camera_photometric,
 *                                                         smx_track_camera_photometric_workspace_bytes, smx_intensity_planes
 *   -- (the term read coarse to fine from pyramids)      smx_intensity_pyramid, smx_intensity_pyramid_bytes,
 *                                                         smx_track_camera_pyramid
 *   TORCH_CHECK -> c10::Error -> RuntimeError             int status + smx_last_error()
 *     depth/stereo_matching.cc:13-15
 *
 * Conventions
 *   - All image pointers are DEVICE pointers on the engine's device (cfg.device_id),
 *     row-major float32 (or uint8 for *_u8), contiguous.  `stream` is a hipStream_t
 *     (NULL = the legacy default stream, which is what the reference launches on).
 *   - Alignment.  Image, map, table and output operands need only the alignment of their
 *     element type (1 byte for uint8, 4 for float32 and int32 operands, 8 for double): a
 *     contiguous view that starts anywhere inside a larger buffer is a valid operand.
 *     A caller-supplied workspace must be 256-byte aligned: that is what hipMalloc (and
 *     torch's allocator) return and the rounding of the layouts inside it, which hold
 *     8-byte values and atomics.  Every entry that takes a workspace (smx_filter_speckles,
 *     smx_fill_invalid, smx_weighted_median, smx_wls_filter, smx_sgm,
 *     smx_sgm_with_right_map, smx_reproject_points, smx_voxel_downsample, smx_project_points,
 *     smx_tsdf_integrate, smx_tsdf_extract_points, smx_tsdf_extract_triangles,
 *     smx_tsdf_raycast, smx_track_camera, smx_track_camera_photometric, smx_track_camera_pyramid) returns
 *     SMX_ERR_INVALID_ARG for a non-NULL workspace that is not, before any device call.
 *   - Calls enqueue work and return without synchronising (like the reference).
 *   - One engine = one device + one set of intermediate buffers: calls on the same
 *     engine must be serialised by the caller (the reference object is not thread-safe
 *     either).  Different engines may be driven from different host threads.
 *   - Output is the full-resolution disparity map [H][W] float32 in full-res pixels,
 *     including the min_disparity offset (reference stereo_matching.cc:42).
 *   - Return value: SMX_OK (0) or a negative smx_status; the message for the calling
 *     thread's last failure is returned by smx_last_error().
 */
#ifndef STEREO_MI355X_H
#define STEREO_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMX_ABI_VERSION 4   /* 2: smx_config.overlap_min_pairs (was reserved[0]), SMX_STREAM_ENGINE, smx_join, smx_overlap_lanes, smx_get_match_geometry;
                               3: smx_config.exact_filter = 1 (always filtered), smx_build_features, smx_get_route_info;
                               4: smx_config.fp_convention (was reserved[0]) */

typedef enum smx_status {
    SMX_OK = 0,
    SMX_ERR_INVALID_ARG = -1,
    SMX_ERR_INVALID_CONFIG = -2,
    SMX_ERR_HIP = -3,
    SMX_ERR_OUT_OF_MEMORY = -4,
    SMX_ERR_UNSUPPORTED = -5
} smx_status;

/* How the cost-volume / aggregation kernel sums (results are identical whenever both apply):
 *   EXACT_ORDER  every box sum is accumulated tap by tap in the reference's order
 *                (multi_block_matching_cost_aggregation.cu:58-85): bit-exact for ANY input.
 *   FAST_GRID    separable running sums; bit-exact iff every pooled pixel is a multiple of
 *                1/K^2 in [0,255] with K in {1,2,4,8} (e.g. integer-valued gray), because
 *                then every partial sum is exactly representable in float32 in any order.
 *   AUTO         the prologue kernel checks that condition on the device and the engine
 *                runs FAST_GRID when it holds, EXACT_ORDER otherwise (always bit-exact).
 *                The RGB entries go straight to EXACT_ORDER (gray computed from RGB is
 *                practically never on the grid), the u8 gray entries straight to FAST_GRID. */
typedef enum smx_match_mode {
    SMX_MATCH_AUTO = 0,
    SMX_MATCH_EXACT_ORDER = 1,
    SMX_MATCH_FAST_GRID = 2
} smx_match_mode;

/* Floating-point convention: how the three sums of products of the path -- step 1, `0.2989 R + 0.5870 G + 0.1140 B`
 * (imageops/kernels/rgb_to_grayscale.cu:24-28), and the sums `a` and `b` of the parabola
 * (depth/kernels/device_functions.cuh:39-40) -- are evaluated.  Nothing else on the path has a multiply feeding an add.
 * The reference's sources do not fix this: depth/setup.py:4-23 passes no nvcc flags, so a CUDA build of the reference
 * contracts a*b+c (nvcc defaults to --fmad=true) and WHICH products it fuses is the compiler's choice.  An add can fuse
 * with at most one of the multiplies that feed it; for `(p1 + p2) + p3`, p_k = a_k * b_k, that leaves six evaluations:
 *   SOURCE        (rn(p1) + rn(p2)) + rn(p3)          no contraction (nvcc --fmad=false); the default
 *   FMA_FIRST     fma(a3,b3, fma(a1,b1, rn(p2)))      the operand order of LLVM's DAG combiner (fadd (fmul x y) z ->
 *                                                     fma x y z is tried first): what an NVVM-based nvcc most plausibly emits
 *   FMA_SECOND    fma(a3,b3, fma(a2,b2, rn(p1)))      every `+ p` fused, left to right
 *   FMA_OUTER     fma(a3,b3, rn(p1) + rn(p2))
 *   FMA_FIRST_IN  fma(a1,b1, rn(p2)) + rn(p3)
 *   FMA_SECOND_IN fma(a2,b2, rn(p1)) + rn(p3)
 * Integer-valued gray inputs with min_disparity = 0 (the BASELINE configurations) give the same bits under all six;
 * RGB input and min_disparity > 0 (the reference's defaults) do not (sensitivity table).  A holder of
 * outputs of a CUDA build picks the convention that reproduces them (tests/test_from_reference.py does it by itself).
 * A compiler chooses per expression: gcc 11 -O2 -mfma -ffp-contract=fast compiles the reference's text to FMA_OUTER in
 * step 1 and FMA_SECOND in the parabola.  SMX_FP_MIXED(step1, parabola) names the two sites separately; a plain value
 * means the same evaluation at both.  (`a` and `b` of the parabola always share one.) */
#define SMX_FP_MIXED(step1, parabola) ((step1) | (((parabola) + 1) << 3))
#define SMX_FP_STEP1(c)    ((c) & 7)
#define SMX_FP_PARABOLA(c) (((c) >> 3) ? ((c) >> 3) - 1 : ((c) & 7))
#define SMX_FP_VALID(c)    ((c) >= 0 && ((c) & 7) < SMX_FP_CONVENTIONS && ((c) >> 3) <= SMX_FP_CONVENTIONS)
typedef enum smx_fp_convention {
    SMX_FP_SOURCE = 0,
    SMX_FP_FMA_FIRST = 1,
    SMX_FP_FMA_SECOND = 2,
    SMX_FP_FMA_OUTER = 3,
    SMX_FP_FMA_FIRST_IN = 4,
    SMX_FP_FMA_SECOND_IN = 5,
    SMX_FP_CONVENTIONS = 6
} smx_fp_convention;

/* First 11 fields mirror reference stereo_matching_configuration.hh:5-17 field for field. */
typedef struct smx_config {
    uint32_t height;            /* 1080 */
    uint32_t width;             /* 1920 (the pybind layer defaults to 1980, torch_extension_module.cc:10) */
    uint32_t downscale_factor;  /* 2    */
    int32_t  min_disparity;     /* 75   */
    int32_t  max_disparity;     /* 262  */
    uint32_t ncc_patch_radius;  /* 1    */
    uint32_t sad_patch_radius;  /* 5    */
    uint32_t threshold;         /* 5    */
    int32_t  small_mbm_radius;  /* 1    */
    int32_t  mid_mbm_radius;    /* 4    */
    int32_t  large_mbm_radius;  /* 10   (supported: small, mid <= large and the exact-order kernel's 16x64 tile
                                           with a halo of large + ncc radius must fit 64 KB of LDS, i.e.
                                           large <= 18 at ncc radius 1, <= 17 at 2, <= 16 at 4, <= 13 at 8;
                                           beyond that smx_create returns SMX_ERR_UNSUPPORTED) */
    /* engine options (no counterpart in the reference) */
    int32_t  device_id;         /* HIP device ordinal, default 0 */
    int32_t  max_batch;         /* pairs accepted by one *_batch call, default 1 */
    int32_t  match_mode;        /* smx_match_mode, default SMX_MATCH_AUTO */
    int32_t  overlap_min_pairs; /* stream lanes (see SMX_STREAM_ENGINE): smallest engine-stream call that is split over the
                                   two lanes; 0 = default (twice the smallest batch that fills the chip with the throughput shape of the
                                   aggregation kernel: 26 pairs at 1242x375; or SMX_OVERLAP_MIN_PAIRS from the environment), -1 = never */
    int32_t  exact_filter;      /* exact-order kernel for off-grid input (RGB entries), batches: 0 = default (content-aware:
                                   the filtered route -- a cheap pass over all disparities bounds which of them can hold the
                                   maximum, only those are evaluated in the reference's order, same bits, k_match_filter.h --
                                   while its candidate sets stay small; the dense kernel once a call reported that they cover
                                   most of the range, as on real scenes; re-probed every 16..64 calls of that kind -- RGB batches large
                                   enough for the filtered route; other calls do not count; smx_get_route_info),
                                   1 = always filtered, -1 = always dense */
    int32_t  fp_convention;     /* smx_fp_convention or SMX_FP_MIXED(step1, parabola), default SMX_FP_SOURCE */
    int32_t  reserved[3];       /* must be 0 */
} smx_config;

typedef struct smx_dims {
    int32_t H, W, K, h, w, dmin, dmax, Dd;   /* reference device_buffer.cc:3-12 */
} smx_dims;

typedef struct smx_engine smx_engine;

/* Intermediates retrievable for parity tests (smx_get_intermediate). */
typedef enum smx_stage {
    SMX_STAGE_GRAY_LEFT = 0,    /* [H][W]    f32 (RGB and u8 entries; the f32 gray entry keeps none:
                                                INVALID_ARG, the planes are the caller's own buffers)  */
    SMX_STAGE_GRAY_RIGHT = 1,
    SMX_STAGE_DOWN_LEFT = 2,    /* [h][w]    f32                                       */
    SMX_STAGE_DOWN_RIGHT = 3,
    SMX_STAGE_WTA = 4,          /* [h][w]    f32  float(arg) + dmin (step 5)           */
    SMX_STAGE_MBM_COSTS = 5,    /* [3][h][w] f32  AGG at (d, d+1, d-1) as step 6 reads them (secondary_matching.cu:28-31:
                                   absolute disparities through pad_index, flat memory) */
    SMX_STAGE_REFINED = 6,      /* [h][w]    f32  after secondary matching (step 6)    */
    SMX_STAGE_AGG_VOLUME = 7,   /* [h][w][Dd] f32; exists only for min_disparity/K > disparity count or non-default radii with
                                   min_disparity > 0 (otherwise smx_stage_bytes() = 0: the three costs step 6 reads are
                                   looked up sparsely, SMX_STAGE_MBM_COSTS holds them for any min_disparity) */
    SMX_STAGE_GRID_FLAG = 8     /* [1] int32: 0 = pooled inputs on the exact grid      */
} smx_stage;

int         smx_abi_version(void);
void        smx_config_default(smx_config *cfg);
int         smx_get_dims(const smx_config *cfg, smx_dims *dims);
const char *smx_last_error(void);

int  smx_create(const smx_config *cfg, smx_engine **out_engine);
void smx_destroy(smx_engine *engine);

/* One pair.  left/right: [3][H][W] f32 (R,G,B planes).  out: [H][W] f32. */
int smx_compute_rgb(smx_engine *engine, const float *left_chw, const float *right_chw,
                    float *out_hw, void *stream);
/* One pair, grayscale entry (skips reference step 1).  left/right: [H][W]. */
int smx_compute_gray(smx_engine *engine, const float *left_hw, const float *right_hw,
                     float *out_hw, void *stream);
int smx_compute_gray_u8(smx_engine *engine, const uint8_t *left_hw, const uint8_t *right_hw,
                        float *out_hw, void *stream);
/* n independent pairs (1 <= n <= cfg.max_batch), densely packed [n][...]: one set of launches on `stream`
 * (or, with stream = SMX_STREAM_ENGINE, on the engine's stream lanes -- see below). */
int smx_compute_gray_batch(smx_engine *engine, int n, const float *left_nhw,
                           const float *right_nhw, float *out_nhw, void *stream);
int smx_compute_rgb_batch(smx_engine *engine, int n, const float *left_nchw,
                          const float *right_nchw, float *out_nhw, void *stream);
/* ... straight from the image decoder: uint8 batches (a quarter of the bytes over PCIe / HBM). */
int smx_compute_gray_u8_batch(smx_engine *engine, int n, const uint8_t *left_nhw,
                              const uint8_t *right_nhw, float *out_nhw, void *stream);
int smx_compute_rgb_u8_batch(smx_engine *engine, int n, const uint8_t *left_nchw,
                             const uint8_t *right_nchw, float *out_nhw, void *stream);

/* Copies an intermediate of pair `pair_index` of the LAST call into dst (device pointer,
 * `bytes` must equal the stage size) on `stream`.  Test/debug facility.  After an LR call of n pairs
 * (smx_compute_lr_*, below) the last call is the one of 2n internal pairs: index i < n is (L_i, R_i), index n + i is
 * the mirrored pair (flip R_i, flip L_i), so e.g. SMX_STAGE_WTA of n + i is the arg-max map of the right view, mirrored. */
int    smx_get_intermediate(smx_engine *engine, int stage, int pair_index, void *dst,
                            size_t bytes, void *stream);
size_t smx_stage_bytes(const smx_engine *engine, int stage);

/* Which aggregation kernel the last call enqueued: SMX_MATCH_EXACT_ORDER, SMX_MATCH_FAST_GRID,
 * or SMX_MATCH_AUTO when both were enqueued and the device-side flag selects. */
int smx_last_match_mode(const smx_engine *engine);

/* Stream lanes.  `stream` argument of the compute entries: run on the library's own two streams (one pair per device,
 * shared by the engines of that device, created in the highest stream-priority pool so that they sit on two hardware
 * queues of their own) instead
 * of a caller's.  Engine-stream calls are ordered against the engine's other calls only where they share memory: the
 * engine keeps its two lanes apart wherever they would touch the same pairs of its buffers or overlapping `out`
 * ranges (two calls that write the same output are ordered and the later one wins, as on one stream; frames that are in
 * flight together need outputs of their own to run side by side), and every engine-stream call comes behind the engine's
 * last call on a caller's stream.  The inputs must be complete when the call is made and stay untouched, and the outputs are defined once smx_join() has ordered a
 * stream behind them (a later call on a caller's stream, smx_get_intermediate and smx_destroy join by
 * themselves).  A call of at least overlap_min_pairs pairs (smx_config; default: see there) is enqueued as two
 * halves, one per lane stream, over disjoint slices of the engine's buffers (independent pairs: the same
 * bits); a smaller call that needs at most half of the engine's pair slots (2 n <= max_batch) goes to the two lanes
 * alternately, on alternate halves of the buffers, so that consecutive small calls -- single frames -- run side by side
 * (an engine created with max_batch = 2 pipelines one-pair calls: 35 k instead of 21 k calls/s at 1242x375).
 * Consecutive calls then pipeline: one half's bandwidth-bound launches and the thin last round of
 * its aggregation kernel run beside the other half's aggregation kernel, across call boundaries (the
 * reference runs its frames serially on one stream, depth_estimation_pipeline_runner.py:51-52). */
#define SMX_STREAM_ENGINE ((void *)(intptr_t)-1)
/* Makes `stream` wait for everything enqueued with SMX_STREAM_ENGINE so far (no host synchronisation). */
int smx_join(smx_engine *engine, void *stream);

/* Stream capture (HIP graphs): a call on a capturing caller stream is captured like any other work (no lane is
 * involved).  While the engine has unjoined SMX_STREAM_ENGINE work, a call / smx_join / smx_get_intermediate on a
 * capturing stream returns SMX_ERR_UNSUPPORTED (the capture would have to wait for work outside of it): join on a
 * non-capturing stream first.  Ordering a graph LAUNCH against the engine's own streams is the caller's business. */

/* Number of stream lanes (1 or 2) an SMX_STREAM_ENGINE call with n pairs runs on. */
int smx_overlap_lanes(const smx_engine *engine, int n);

/* How the FAST_GRID aggregation kernel of a call with n pairs tiles the (row, column, disparity) volume:
 * every wave marches `rows_marched` rows for `band_rows` rows of output and spends 64 lanes on
 * `columns_per_wave` output columns (the rest is halo for the 21-wide / 21-high boxes of
 * multi_block_matching_cost_aggregation.cu:54-88).  useful_fraction = output (pixel, disparity) cells /
 * (lane, row, disparity) cells marched by the dense first pass, over the whole launch.  The plan is the one the engine's
 * LAST call used (stream lanes or a caller's stream: the lanes take the throughput shape from fewer pairs on); for a
 * call the lanes split, `workgroups` counts one half's launch.  The geometry describes the plan of the kernel's SPARSE
 * form: a batch call that takes the dense form where the sparse plan has 32-row bands launches 27-row bands. */
typedef enum smx_match_kernel {
    SMX_KERNEL_EXACT_ONLY = 0,      /* configuration outside the FAST_GRID envelope                         */
    SMX_KERNEL_FAST_WINDOW = 1,     /* one 64-column window per wave, tall bands                             */
    SMX_KERNEL_FAST_SPLIT = 2,      /* few pairs in flight: short bands, disparity range split over 4 waves  */
    SMX_KERNEL_FAST_WIDE = 3        /* reserved (a removed workgroup-wide kernel, NOTES.md): never reported  */
} smx_match_kernel;
typedef struct smx_match_geometry {
    int32_t kernel;                 /* smx_match_kernel */
    int32_t band_rows, rows_marched;
    int32_t waves_per_workgroup, workgroups;
    double  columns_per_wave;       /* average output columns per 64 lanes, image edge included */
    double  useful_fraction;
} smx_match_geometry;
int smx_get_match_geometry(const smx_engine *engine, int n, smx_match_geometry *out);

/* Optional features the library was built with, as a bit set.  No optional feature is currently compiled in: the
 * result is 0.  SMX_FEATURE_EXPERIMENTAL is reserved (it marked builds with two negative-result kernels, since removed;
 * NOTES.md) and never reported. */
#define SMX_FEATURE_EXPERIMENTAL 1
int smx_build_features(void);

/* Launch-plan state that depends on what earlier calls saw.  The kernels publish two hints into pinned host memory
 * without any synchronisation: the candidate density of filtered launches (exact_filter = 0: route choice) and
 * whether the last single f32 gray call was off the exact grid (AUTO: one fused launch while the reports say "on the grid",
 * two gated ones -- the fast kernel and the disparity-split exact-order kernel -- after an "off" report and before the first report).  Every
 * plan produces the same bits; the hints only pick the faster one for the content at hand.  Third hint: how many
 * disparities the sparse second pass of the fast kernel revisited per window (on-grid batches, min_disparity = 0): above
 * ~0.10 of the range the engine switches to the pass that keeps the winner's neighbours as it goes (fast_dense), probing the
 * sparse form every 16..64 calls of that kind (calls whose launch plan has a dense form and whose sparse form reports;
 * calls of any other kind neither count nor take a probe) and returning below ~0.07.  Single frames whose
 * launch plan is the latency shape with 12-row bands follow the same state. */
typedef struct smx_route_info {
    int32_t filter_available;    /* the configuration admits the filtered exact-order route                   */
    int32_t route_dense;         /* 1: off-grid batches currently take the dense exact-order kernel           */
    int32_t last_call_filtered;  /* decision taken for the most recent call (1 also while probing)            */
    int32_t probe_period;        /* calls that can take the filtered route between its probes while route_dense */
    float   candidate_density;   /* evaluated / possible disparity slices of the last reported filtered launch, -1: none yet */
    int32_t offgrid_hint;        /* the last reported single f32 gray call was off (1) / on (0) the exact grid; -1: no report yet */
    int32_t compute_units;       /* multiProcessorCount the launch plans are sized against                    */
    int32_t fast_dense;          /* 1: on-grid batches (min_disparity = 0) currently take the dense form of the fast kernel (windows hold many winners) */
} smx_route_info;
int smx_get_route_info(smx_engine *engine, smx_route_info *out);

/* Opt-in per-kernel timing with HIP events recorded on the caller's stream (the reference's
 * only hook is a wall-clock print, helpers/torch_helpers.py:19-28).  After smx_profile_begin
 * every enqueued kernel is bracketed by two events until `max_calls` calls were recorded;
 * smx_profile_end synchronises those events and returns, per kernel slot, the mean duration
 * in milliseconds and the number of launches averaged (slots: see smx_kernel_slot). */
typedef enum smx_kernel_slot {
    SMX_KERNEL_PROLOGUE = 0,     /* gray + mean pool (steps 1-2)             */
    SMX_KERNEL_MATCH_FAST = 1,   /* cost volume + aggregation + WTA, FAST    */
    SMX_KERNEL_MATCH_EXACT = 2,  /* cost volume + aggregation + WTA, EXACT   */
    SMX_KERNEL_REFINE = 3,       /* secondary matching (step 6)              */
    SMX_KERNEL_FILL = 4,         /* upscale + vertical + horizontal fill     */
    SMX_KERNEL_SLOTS = 5
} smx_kernel_slot;
int smx_profile_begin(smx_engine *engine, int max_calls);
int smx_profile_end(smx_engine *engine, float mean_ms[SMX_KERNEL_SLOTS], int launches[SMX_KERNEL_SLOTS]);

/* "Next" row f2: the evaluation metrics the reference computes on the disparity map right after
 * the path (python/pipeline/depth_estimation_pipeline_metrics.py:18-56, runner.py:82-94), fused
 * into one device pass.  est/gt: [n][pixels] f32 device pointers; mask: [n][pixels] bytes
 * (torch.bool) or NULL, in which case the runner's gt_mask = (gt <= max_disparity) & (gt > 0) is
 * evaluated on the fly.  out_sums: [n][8] doubles on the device, ZEROED by this call and then
 * accumulated: {count, D1 hits, hits for thresholds[0..3], sum |est-gt|, 0}.  metric = sum/count. */
int smx_eval_metrics(int device_id, int n, const float *est, const float *gt, const uint8_t *mask,
                     size_t pixels, float max_disparity, const float thresholds[4], double *out_sums,
                     void *stream);

/* "Next" row f3: what the reference does with the map first (PointCloudSaver,
 * python/pipeline/depth_estimation_pipeline_hooks.py:84-92 + helpers/point_cloud_helpers.py:5-13):
 * depth = baseline_times_focal / disparity for every pixel (depth_hw, may be NULL) and the list of
 * [y, x, depth] for the pixels whose disparity != invalid_disparity, in row-major order
 * (points: room for H*W*3 floats; *count_dev receives the number of points).  workspace: 2*H ints.
 * All pointers are device pointers. */
int smx_disparity_to_points(int device_id, const float *disparity_hw, int H, int W,
                            float baseline_times_focal, float invalid_disparity, float *depth_hw,
                            float *points, int *count_dev, int *workspace, void *stream);

/* uint8 RGB ingestion ([3][H][W] bytes, what torchvision.io.read_image hands the reference's backend
 * before its .float(), cuda_stereo_matching_backend.py:14-15): the u8 -> f32 cast is fused into the
 * prologue kernel.  Same results as smx_compute_rgb on the .float() of the same tensors. */
int smx_compute_rgb_u8(smx_engine *engine, const uint8_t *left_chw, const uint8_t *right_chw,
                       float *out_hw, void *stream);

/* Left-right consistency check: marks the pixels whose match does not point back to them -- occlusions, the band
 * Y < min_disparity along the left edge, mismatches -- with invalid_disparity (the value PointCloudSaver drops,
 * python/pipeline/depth_estimation_pipeline_hooks.py:87-88; smx_disparity_to_points above).  E(L, R) is what the plain
 * entries compute; flip reverses the column axis (every plane of RGB input).
 *   D_L = E(L, R)                                 (the same bits as the plain *_batch entry)
 *   D_R = flip(E(flip R, flip L))                 the map referenced to the right image: the engine's own problem on the
 *                                                 mirrored, swapped pair (same configuration, fp_convention and match_mode)
 *   per pixel (X, Y), float32:
 *     t  = floorf(D_L[X][Y] + 0.5f);  ok = isfinite(t) && t >= 0 && t <= Y
 *     ok = ok && fabsf(D_L[X][Y] - D_R[X][Y - (int)t]) <= max_diff        (NaN D_R: not ok)
 *     out[X][Y] = ok ? D_L[X][Y] : invalid_disparity
 * One call = ONE engine call of 2n internal pairs on `stream` (the aggregation kernel sees twice the pairs) between an
 * input pack / mirror launch and the check launch; its cost is about that of a plain call of 2n pairs.  The packed
 * inputs and raw outputs live in engine-owned scratch, allocated by the first LR call for max_batch pairs of its input
 * format (regrown once for a larger format, never in a steady loop); a first LR call on a capturing stream returns
 * SMX_ERR_UNSUPPORTED (make one outside capture first).  Plain calls give the same bits before and after LR calls.
 * n pairs, same layouts as the *_batch entries, 1 <= n and 2*n <= cfg.max_batch (else SMX_ERR_INVALID_ARG).
 * out: [n][H][W], checked left map.  right_out: [n][H][W] un-checked right-view map D_R, or NULL.  The inputs must not
 * overlap out / right_out, nor out right_out (SMX_ERR_INVALID_ARG).  max_diff must be finite and >= 0, invalid_disparity
 * finite (SMX_ERR_INVALID_ARG).  stream = SMX_STREAM_ENGINE: SMX_ERR_UNSUPPORTED (LR calls run on a caller's stream).
 * Every argument is checked before the device is touched. */
int smx_compute_lr_gray_batch(smx_engine *engine, int n, const float *left_nhw, const float *right_nhw, float *out_nhw,
                              float *right_out_nhw, float max_diff, float invalid_disparity, void *stream);
int smx_compute_lr_gray_u8_batch(smx_engine *engine, int n, const uint8_t *left_nhw, const uint8_t *right_nhw,
                                 float *out_nhw, float *right_out_nhw, float max_diff, float invalid_disparity,
                                 void *stream);
int smx_compute_lr_rgb_batch(smx_engine *engine, int n, const float *left_nchw, const float *right_nchw, float *out_nhw,
                             float *right_out_nhw, float max_diff, float invalid_disparity, void *stream);
int smx_compute_lr_rgb_u8_batch(smx_engine *engine, int n, const uint8_t *left_nchw, const uint8_t *right_nchw,
                                float *out_nhw, float *right_out_nhw, float max_diff, float invalid_disparity,
                                void *stream);
/* Standalone check of maps the caller already has (e.g. from another backend): the same rule, D_R given un-mirrored.
 * left/right/out: [n][H][W] f32 device pointers on device_id; out may alias left (the same buffer), not right.
 * stream: a caller's stream. */
int smx_lr_check(int device_id, int n, int H, int W, const float *left_disp, const float *right_disp, float *out,
                 float max_diff, float invalid_disparity, void *stream);

/* Post-processing of checked maps: speckle filter and background hole fill.  Maps are [n][H][W] float32 on the device;
 * the n maps are independent (nothing connects across map boundaries).  A pixel value d is VALID iff
 * isfinite(d) && d != invalid_disparity (float comparison, so -0.0 == 0.0).
 *
 * Speckle filter:
 *   - Two 4-neighbours p, q of the same map are LINKED iff both are valid and fabsf(d_p - d_q) <= max_diff.  The
 *     subtraction is in float32.  There is no multiply, so there is no contraction question.
 *   - A REGION is a connected component of the linked relation: the transitive closure, 4-connectivity, no wrap-around.
 *   - Every pixel of a region with size <= max_speckle_size becomes invalid_disparity.  This is the <= of
 *     cv::filterSpeckles.  Every other pixel is copied unchanged, bit for bit, including non-valid ones such as NaN
 *     payloads.
 *   - max_speckle_size = 0 is a plain copy.
 *
 * Hole fill (background interpolation), two passes.
 *   Row pass, on the input:
 *   - For each non-valid pixel (x, y), let a be the nearest valid column < y in the same row and b the nearest valid
 *     column > y.
 *   - If both exist, the value is (D[x][a] <= D[x][b]) ? D[x][a] : D[x][b].  The left value wins ties, which pins
 *     -0.0 / +0.0.
 *   - If only one exists, use its value.
 *   - If neither exists, leave the pixel unchanged.
 *   Column pass, on the result of the row pass:
 *   - Every row with at least one valid input pixel is now fully valid.
 *   - For each row with no valid input pixel, let r1 be the nearest non-empty row above and r2 the nearest non-empty
 *     row below.
 *   - If both exist, each pixel takes (D[r1][y] <= D[r2][y]) ? D[r1][y] : D[r2][y].  The row above wins ties.
 *   - If only one exists, copy it.
 *   - If the whole map is non-valid, the map is copied unchanged.
 *
 * Both entries are engine-free.  in / out: [n][H][W] f32 device pointers on device_id; out may be in (in place) but
 * must not overlap it otherwise.  workspace: device memory of at least smx_postprocess_workspace_bytes(n, H, W) bytes,
 * overlapping neither map; its layout is implementation-defined and it holds nothing between calls (any contents give
 * the same result).  Each call enqueues a fixed sequence of launches on `stream` (a caller's stream, not
 * SMX_STREAM_ENGINE), with no host synchronisation and no allocation, so it can be captured into a HIP graph.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL pointer, n < 1, H or W outside 1..32768,
 * max_speckle_size < 0, max_diff not finite or < 0, invalid_disparity not finite, workspace_bytes below the query,
 * the overlaps above, stream == SMX_STREAM_ENGINE. */
size_t smx_postprocess_workspace_bytes(int n, int H, int W);   /* 0 for n < 1 or H, W outside 1..32768 */
int smx_filter_speckles(int device_id, int n, int H, int W, const float *in, float *out, int max_speckle_size,
                        float max_diff, float invalid_disparity, void *workspace, size_t workspace_bytes, void *stream);
int smx_fill_invalid(int device_id, int n, int H, int W, const float *in, float *out, float invalid_disparity,
                     void *workspace, size_t workspace_bytes, void *stream);

/* Image-guided weighted median (Rhemann et al. CVPR 2011; Hosni et al. TPAMI 2013), normally run on the pixels the
 * hole fill wrote.  Every operand is [n][H][W] f32 on the device; the n maps are independent.  VALID is as above.
 *   - Weights are integers.  range_weight[256] and spatial_weight[(radius+1)^2] are host tables of uint16 values in
 *     0..1023.  For a centre p and a sample q at offset (dy, dx) in its window,
 *       w = spatial_weight[|dy| * (radius+1) + |dx|] * range_weight[k],
 *     where a = fabsf(guide[p] - guide[q]) in float32 and k = (isnan(a) || a >= 255) ? 255 : (int)a (truncation).
 *     Every sum of weights is below 2^30, so all sums are exact in uint32 in any order.
 *   - Window: (2 radius + 1)^2 pixels, radius in 1..15, clipped to the map (no padding, no wrap-around).  The SAMPLES
 *     are the window pixels q that are valid in `in` and have w > 0; T is the sum of their weights.
 *   - Filtered set F: with holes == NULL, the pixels valid in `in`; otherwise the pixels NOT valid in `holes` (the
 *     pixels the fill wrote).  Every pixel outside F, and every pixel of F whose T is 0, is copied bit for bit from in.
 *   - Median: with u = bits(d) and key(d) = (u & 0x80000000) ? ~u : (u | 0x80000000) (a total order, -0.0 < +0.0),
 *     out[p] is the sample value with the smallest key K such that 2 * sum(w_q : key(d_q) <= K) >= T.  It is a value
 *     that occurs in the window, so every implementation gives the same bits.
 * out must not overlap in or guide.  out may be exactly holes (overwrite the pre-fill map) but must not overlap it
 * otherwise.  in, holes and guide may alias each other (holes == in: a weighted-median fill of the non-valid pixels,
 * with no background fill before it).  The tables are read during the call (passed by value in the kernel arguments).
 * workspace: NULL or device memory of at least smx_median_workspace_bytes(n, H, W) bytes (which may be 0) overlapping
 * no operand; its contents do not affect the result.  One launch on `stream` (a caller's stream), with no host
 * synchronisation and no allocation, so it can be captured into a HIP graph.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL in, guide, out or table, n < 1, H or W outside
 * 1..32768, radius outside 1..15, a table value above 1023, invalid_disparity not finite, workspace_bytes below the query
 * or workspace NULL with workspace_bytes > 0, the overlaps above, stream == SMX_STREAM_ENGINE. */
size_t smx_median_workspace_bytes(int n, int H, int W);        /* may be 0; 0 for n < 1 or H, W outside 1..32768 */
int smx_weighted_median(int device_id, int n, int H, int W, const float *in, const float *holes, const float *guide,
                        float *out, int radius, const uint16_t range_weight[256], const uint16_t spatial_weight[],
                        float invalid_disparity, void *workspace, size_t workspace_bytes, void *stream);

/* Image-guided weighted least squares filter: the fast global smoother of Min et al. (TIP 2014) as a confidence-weighted
 * disparity filter.  It makes a checked map dense, smooth inside surfaces, with edges that follow the guide's.  Every
 * operand is [n][H][W] f32 on the device; the n maps are independent.  VALID is as above.
 *   1. Confidence: c(p) = 0 where p is not valid; otherwise 1.0f with confidence == NULL, else
 *      (conf > 0) ? fminf(conf, 1.0f) : 0.0f (a NaN confidence gives 0).
 *   2. Planes: U(p) = valid ? d * c : 0.0f (one float32 product), V(p) = c(p).
 *   3. Edge weight between horizontal or vertical neighbours p, q: a = fabsf(guide[p] - guide[q]) in float32,
 *      k = (isnan(a) || a >= 255) ? 255 : (int)a (as in the weighted median), w = range_weight[k]; range_weight is a host
 *      table of 256 finite float32 values in [0, 1].
 *   4. Iterations t = 0 .. T-1, T = num_iterations in 1..8, lambda = lambdas[t] (host table of finite float32 values,
 *      0 <= lambda <= 2^20): first every row of U and every row of V is solved, then every column of U and of V; each
 *      result replaces its line.
 *   5. One line solve of f_0 .. f_{N-1} with guide g_0 .. g_{N-1}: s_j = lambda * w(g_j, g_{j+1}) for j < N-1;
 *      L_j = j > 0 ? s_{j-1} : 0, R_j = j < N-1 ? s_j : 0, b_j = (1.0f + L_j) + R_j.  Forward: r_0 = 1.0f / b_0,
 *      e_0 = R_0 * r_0, y_0 = f_0 * r_0; for j >= 1 r_j = 1.0f / (b_j - L_j * e_{j-1}), e_j = R_j * r_j,
 *      y_j = (f_j + L_j * y_{j-1}) * r_j.  Back: x_{N-1} = y_{N-1}, x_j = y_j + e_j * x_{j+1}.  This is the Thomas
 *      algorithm for (I + lambda A_w) x = f.  Every operation is one float32 round-to-nearest with no fused operation,
 *      the division is the correctly rounded one, and denormals are kept.  In exact arithmetic every pivot is
 *      >= 1 + R_j; lambda <= 2^20 keeps the rounded pivots well above 0.
 *   6. out(p) = (V > min_weight) ? U / V : invalid_disparity (a NaN V gives invalid_disparity); a NaN quotient is stored
 *      as 0x7FC00000.  Every pixel is rewritten, valid ones included.
 *   Consequences: lambda = 0 gives back every valid pixel's value (bit for bit, except that a -0.0 may come back as
 *   +0.0) and marks the others invalid; a guide edge whose weight is 0 decouples its two sides exactly.
 * in, confidence (NULL: every valid pixel has confidence 1) and guide may alias each other.  out may be exactly in but
 * must not overlap it otherwise, nor confidence or guide.  The tables are read during the call (passed by value in the
 * kernel arguments).  workspace: device memory of at least smx_wls_workspace_bytes(n, H, W) bytes overlapping no
 * operand; with R(v) = v rounded up to a multiple of 256 the size is 3 R(4 n H W) (the U, V and forward-sweep planes);
 * its contents on entry do not matter.  2 num_iterations launches on `stream` (a caller's stream), with no host
 * synchronisation and no allocation, so the call can be captured into a HIP graph.  Engine-free: device_id only selects
 * the device.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL in, guide, out, lambdas or range_weight, n < 1, H
 * or W outside 1..32768, num_iterations outside 1..8, a lambda that is not finite in [0, 2^20], a range weight that is
 * not finite in [0, 1], min_weight not finite or < 0, invalid_disparity not finite, a NULL workspace or workspace_bytes
 * below the query, the overlaps above, stream == SMX_STREAM_ENGINE. */
size_t smx_wls_workspace_bytes(int n, int H, int W);           /* 0 for n < 1 or H, W outside 1..32768 */
int smx_wls_filter(int device_id, int n, int H, int W, const float *in, const float *confidence, const float *guide,
                   float *out, int num_iterations, const float lambdas[], const float range_weight[256],
                   float min_weight, float invalid_disparity, void *workspace, size_t workspace_bytes, void *stream);

/* Per-pixel confidence in [0, 1] of a disparity map, the input of smx_wls_filter's confidence and of any thresholding
 * downstream.  Every operand is [n][H][W] f32 on the device; the n maps are independent.  VALID is as above.  For a
 * pixel (X, Y) with d = D_L[X][Y]:
 *   1. d not VALID: conf = 0.0f.
 *   2. LR term.  right_disp == NULL: c_lr = 1.0f.  Otherwise t = floorf(d + 0.5f); !(t >= 0 && t <= Y): conf = 0 (the
 *      index rule of smx_lr_check); r = D_R[X][Y - (int)t]; r not VALID: conf = 0; otherwise e = fabsf(d - r) and
 *      c_lr = fmaxf(0.0f, 1.0f - e / lr_scale).
 *   3. Texture term.  guide == NULL: c_tex = 1.0f.  Otherwise, over the (2R+1) x (2R+1) guide values around the pixel
 *      (R = radius, 1..15; coordinates clamped into the image), range = max - min of the non-NaN values (one float32
 *      subtraction; -0.0 and +0.0 count as equal, so a zero range is +0.0) and c_tex = fminf(1.0f, range / texture_scale);
 *      c_tex = 0 when every value of the window is NaN or the range is NaN (+inf - +inf).  Max and min do not depend on
 *      the order of evaluation, so the result does not depend on how an implementation splits the window.
 *   4. conf = c_lr * c_tex (one float32 product).  Every zero above is +0.0f.
 * Every operation is one float32 round-to-nearest with no fused operation, the divisions are the correctly rounded
 * ones and denormals are kept, so every implementation gives the same bits.  Suggested starting points, not tuned
 * values: lr_scale = 1 (disparity px), radius = 2, texture_scale = 10 (gray levels).
 * right_disp (the un-checked right-view map, e.g. the right_out of smx_compute_lr_*_batch or smx_sgm_with_right_map)
 * and guide (e.g. the left gray plane) may each be NULL; the inputs may alias each other; out must not overlap any of
 * them.  One launch on `stream` (a caller's stream), with no host synchronisation and no allocation, so the call can be
 * captured into a HIP graph.  Engine-free: device_id only selects the device.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL left_disp or out, n < 1, H or W outside 1..32768,
 * radius outside 1..15 with a guide, lr_scale or texture_scale not finite and > 0, invalid_disparity not finite, the
 * overlaps above, stream == SMX_STREAM_ENGINE. */
int smx_confidence_map(int device_id, int n, int H, int W, const float *left_disp, const float *right_disp,
                       const float *guide, int radius, float lr_scale, float texture_scale, float invalid_disparity,
                       float *out, void *stream);

/* Motion-gated temporal filter of disparity-map streams: blends each pixel's new measurement with its history where the
 * guide image has not changed around it, and resets everywhere else (no motion compensation, so no ghosting).  Every
 * operand is [n][H][W] f32 on the device; the n maps are n independent streams.  VALID is as above.  Inputs: disp (d),
 * confidence (c, may be NULL), guide (g, the current left gray plane), prev_guide (G, the previous frame's).  State, read
 * and written at the same pixel only: state_disp (D), state_weight (A); start it with A = 0 (D is then never read as a
 * value).  Outputs: out, and guide_out (may be NULL), which receives a copy of g for the next call.  Per pixel p:
 *   1. Motion.  e(q) = fabsf(g(q) - G(q)), q clamped into the image; R = motion_radius.  Each window row gives
 *      r(dy) = (...(e(-R) + e(-R+1)) + ...) + e(R), summed in dx order; then S = (...(r(-R) + r(-R+1)) + ...) + r(R),
 *      summed in dy order.  STATIC iff S <= T with T = motion_threshold * (float)(2R+1)^2 (one float32 product).  A NaN
 *      or inf anywhere in the window makes S NaN or +inf, so the pixel is not STATIC (while T is finite).  The fixed
 *      order makes the sum separable and reproducible; an implementation must not use another.
 *   2. Measurement weight.  w = 0 if d is not VALID; otherwise w = 1.0f with confidence == NULL, else
 *      (c > 0) ? fminf(c, 1.0f) : 0.0f (step 1 of smx_wls_filter).
 *   3. a = A * decay; hist = (a > 0) && STATIC && VALID(D).
 *   4. VALID(d), hist and fabsf(d - D) <= max_diff: out = (a*D + w*d) / (a + w), A' = fminf(a + w, max_weight).
 *      VALID(d) otherwise (no history, or disagreement): out = d, A' = w.
 *      d not VALID, hist and a >= min_weight: out = D, A' = a (hold, with a decaying weight).
 *      Otherwise: out = invalid_disparity, A' = 0.
 *   5. D' = out; guide_out = g if guide_out is non-NULL.
 * Every operation is one float32 round-to-nearest with no fused operation, the division is the correctly rounded one
 * and denormals are kept, so every implementation gives the same bits.  With A = 0 everywhere (after a reset) the call
 * returns d at the VALID pixels and invalid_disparity elsewhere.  Suggested starting points, not tuned values:
 * motion_radius = 1, motion_threshold = 4 (gray levels per window pixel), decay = 0.8, max_diff = 1 (disparity px),
 * max_weight = 8, min_weight = 0.25.
 * Ranges: motion_radius 0..7; motion_threshold finite and >= 0; decay in (0, 1]; max_diff finite and >= 0; max_weight
 * finite and > 0; min_weight finite and >= 0; invalid_disparity finite.  Overlaps: the inputs may alias each other;
 * out is exactly disp or does not overlap it, and does not overlap any other operand; state_disp and state_weight do not
 * overlap each other or any input; guide_out does not overlap guide, prev_guide or any other operand.  One launch on
 * `stream` (a caller's stream), with no host synchronisation and no allocation, so the call can be captured into a HIP
 * graph.  Engine-free: device_id only selects the device.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL disp, guide, prev_guide, state_disp, state_weight or
 * out, n < 1, H or W outside 1..32768, a parameter outside its range, the overlaps above, stream == SMX_STREAM_ENGINE. */
int smx_temporal_filter(int device_id, int n, int H, int W, const float *disp, const float *confidence,
                        const float *guide, const float *prev_guide, float *state_disp, float *state_weight,
                        float *guide_out, float *out, int motion_radius, float motion_threshold, float decay,
                        float max_diff, float max_weight, float min_weight, float invalid_disparity, void *stream);

/* Rectification of raw frames: a bilinear remap through a precomputed map, with an integer-defined rule, so that every
 * implementation gives the same bits.
 *   - Map: [H_out][W_out][2] int32, interleaved (x, y), in units of 1/32 pixel (5 fractional bits, OpenCV's
 *     INTER_BITS).  The map is input data: every int32 value is legal and defined, and no value reads outside the input.
 *   - Per output pixel, with (qx, qy) its map entry: x0 = qx >> 5, y0 = qy >> 5 (arithmetic shifts: floor), fx = qx & 31,
 *     fy = qy & 31.  The four taps are (y0, x0), (y0, x0+1), (y0+1, x0), (y0+1, x0+1), with the weights
 *     w00 = (32-fx)(32-fy), w01 = fx(32-fy), w10 = (32-fx)fy, w11 = fx*fy, which sum to 1024.  x0 + 1 and y0 + 1 are at
 *     most 2^26: no tap coordinate overflows.
 *   - SMX_BORDER_CONSTANT: a tap outside the input reads border_value (OpenCV's BORDER_CONSTANT, per tap).
 *     SMX_BORDER_REPLICATE: each tap coordinate is clamped to the input.
 *   - uint8: out = (w00 p00 + w01 p01 + w10 p10 + w11 p11 + 512) >> 10 in integers: the exact bilinear value, rounded
 *     half up.  border_value must be an integer in 0..255.
 *   - float32: out = ((w00 p00 + w01 p01) + (w10 p10 + w11 p11)) * 0.0009765625f, every operation a float32
 *     round-to-nearest with no fused operation.  A tap whose weight is 0 is not read and contributes +0.0, so an inf or
 *     NaN behind a zero weight does not reach the result.  A NaN result is stored as the canonical quiet NaN
 *     0x7FC00000, whatever the sign and payload of the NaNs it came from.  border_value must be finite.
 *   - Not OpenCV bit for bit: OpenCV's 8-bit remap uses 15-bit rounded weight tables; this rule is the exact rational
 *     value, rounded.
 * Images are planar [n][C][H][W] (as the engine's CHW entries), C in 1..4, every channel with the same taps; each view
 * has its own map, shared by the n images of that view.  left_* is required; right_in, right_map and right_out are all
 * NULL (left view only) or all non-NULL.  One launch on `stream` (a caller's stream), with no host synchronisation and
 * no allocation, so it can be captured into a HIP graph.  Engine-free: device_id only selects the device.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL left operand, a partially-NULL right triple, n < 1
 * (or n frames larger than the address space),
 * a size outside 1..32768, channels outside 1..4, an unknown dtype or border mode, a non-finite border_value or, for
 * uint8, one that is not an integer in 0..255, an output overlapping any input or map or the other output,
 * stream == SMX_STREAM_ENGINE. */
#define SMX_BORDER_CONSTANT  0
#define SMX_BORDER_REPLICATE 1
#define SMX_DTYPE_U8  0
#define SMX_DTYPE_F32 1
int smx_remap_pairs(int device_id, int n, int channels, int dtype, int H_in, int W_in, int H_out, int W_out,
                    const void *left_in, const void *right_in, const int32_t *left_map, const int32_t *right_map,
                    void *left_out, void *right_out, int border_mode, float border_value, void *stream);

/* Right-view synthesis head: everything Deep3D does after the network's last layer, in one launch.  The network (the
 * caller's) leaves a soft-maxed probability volume at low resolution; the head upsamples it bilinearly by an integer
 * factor, weighs D shifted copies of the left frame with it, sums over the disparity axis and rescales to 0..255.
 * Neither the upsampled volume nor the stack of shifted copies is ever stored.
 *   - prob: [n][D][h][w] f32 (P).  left: [n][C][H][W], SMX_DTYPE_F32 or SMX_DTYPE_U8, H = h * S, W = w * S.
 *     out: [n][C][H][W] f32.  S = scale (1..16; the reference's is 4), D in 1..256 (the reference's is 65), C 1 or 3.
 *   - Bilinear source indices, in integers (the half-pixel rule of align_corners = False), per axis, for output index t
 *     and input length len:  u = max(2t + 1 - S, 0);  i0 = u / 2S;  i1 = min(i0 + 1, len - 1);
 *     l1 = (float)(u % 2S) / (float)(2S) (one correctly rounded division; exact for S a power of two);  l0 = 1.0f - l1.
 *     The row X gives (r0, r1, a0, a1), the column Y gives (c0, c1, b0, b1).
 *   - For d = 0, 1, ..., D-1 in this order, while Y + d < W (later terms are skipped, not added as zeros):
 *       top = b0 * P[d][r0][c0] + b1 * P[d][r0][c1];   bot = b0 * P[d][r1][c0] + b1 * P[d][r1][c1];
 *       q = a0 * top + a1 * bot;   for each channel c:  acc_c = acc_c + q * v_c,
 *     with v_c = left[c][X][Y + d] for f32 and (float)byte / 255.0f (the correctly rounded division; the reference's
 *     `/ 255.0`) for u8; acc_c starts at +0.0f.
 *   - Rescale: out = fminf(fmaxf(acc_c * 255.0f + 0.5f, 0.0f), 255.0f).  The reference writes `x * 255 + 0.5` with a
 *     double literal: the float32 product plus 0.5 is exact in double, so its one rounding back to float gives the bits
 *     of the float32 addition.
 * Every operation is one float32 round-to-nearest with no fused operation, denormals are kept, and a NaN follows
 * fmaxf / fminf (a NaN sum is stored as 0).  The order of the sum over d is part of the rule, so every implementation
 * gives the same bits, however it tiles the frame or splits the disparity axis.  Against the reference's torch
 * expression (interpolate, shifted stack, mul, sum) the result differs only by that expression's own summation order:
 * at most 255 * 2 (D + 6) 2^-24, 1.4e-4 measured at D = 65.
 * prob and left may alias each other; out must not overlap either.  One launch on `stream` (a caller's stream), with no
 * workspace, no host synchronisation and no allocation, so the call can be captured into a HIP graph.  Engine-free:
 * device_id only selects the device.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL prob, left or out, n < 1 (or n frames larger than
 * the address space), channels not 1 or 3, an unknown dtype, D outside 1..256, scale outside 1..16, h or w < 1 or
 * h * scale or w * scale > 32768, the overlaps above, stream == SMX_STREAM_ENGINE. */
int smx_synthesize_right_view(int device_id, int n, int channels, int dtype, int D, int h, int w, int scale,
                              const float *prob, const void *left, float *out, void *stream);

/* The synthesis head for training: the view a loss sees, and the gradient of the volume.  Notation, operands, ranges
 * and argument rules are smx_synthesize_right_view's.
 *   - smx_synthesis_head_forward (the training form): that rule up to and including acc_c, without the rescale step:
 *     view[c][X][Y] = acc_c, float32, unclamped (0..1 for a soft-maxed volume and a frame in 0..1).  The output of
 *     smx_synthesize_right_view is the rescale of this view, bit for bit.  view: [n][C][H][W] f32.
 *   - smx_synthesis_head_backward: given g = dL/dview as grad_view [n][C][H][W] f32, grad_prob [n][D][h][w] f32 =
 *     dL/dprob.  left gets no gradient.  For each frame and each d = 0 .. D-1:
 *       Plane gradient, for the columns with Y + d < W:  G[X][Y] = g_0 * v_0[X][Y + d];  for C = 3 then
 *         G = G + g_1 * v_1[X][Y + d];  G = G + g_2 * v_2[X][Y + d]  (each product and each sum rounded).  Columns with
 *         Y + d >= W contribute no term below: they are skipped, not added as zeros, as in the forward rule.
 *       Horizontal transpose, for every row X and low-resolution column j:  T[X][j] starts at +0.0f; for
 *         Y = 0, 1, ..., W-1 in this order:  if c0[Y] == j:  T = T + b0[Y] * G[X][Y];  then, if c1[Y] == j:
 *         T = T + b1[Y] * G[X][Y].  A column whose two taps are the same cell adds both terms, b0 first; a term with a
 *         zero weight is still added.
 *       Vertical transpose, for every cell (i, j):  grad_prob[d][i][j] starts at +0.0f; for X = 0, 1, ..., H-1 in this
 *         order:  if r0[X] == i:  acc = acc + a0[X] * T[X][j];  then, if r1[X] == i:  acc = acc + a1[X] * T[X][j].
 *     For d >= W the plane is all zeros.  The indices that reach a cell are contiguous: 2 scale of them in the interior,
 *     at most 2 scale + scale / 2 at the borders.
 * Every operation is one float32 round-to-nearest with no fused operation, denormals are kept, NaNs and infinities
 * spread as the operations say.  The order of each sum is part of the rule, so every implementation gives the same
 * bits, whatever its tiles, its chunks of the disparity axis, or whether it computes a G once or once per cell that
 * uses it.  In exact arithmetic the rule is the gradient of the training form; in float32 each value lies within
 * (C + terms per row cell + terms per column cell + 2) 2^-24 of the sum of its terms' absolute values.
 * An output must not overlap an input; inputs may alias each other.  One launch each on `stream` (a caller's stream),
 * with no workspace, no atomics, no host synchronisation and no allocation, so the calls can be captured into a HIP
 * graph.  Engine-free: device_id only selects the device.
 * SMX_ERR_INVALID_ARG, checked before the device is touched, in smx_synthesize_right_view's order: a NULL operand,
 * n < 1 (or n frames larger than the address space), channels not 1 or 3, an unknown dtype, D outside 1..256, scale
 * outside 1..16, h or w < 1 or h * scale or w * scale > 32768, the overlaps above, stream == SMX_STREAM_ENGINE. */
int smx_synthesis_head_forward(int device_id, int n, int channels, int dtype, int D, int h, int w, int scale,
                               const float *prob, const void *left, float *view, void *stream);
int smx_synthesis_head_backward(int device_id, int n, int channels, int dtype, int D, int h, int w, int scale,
                                const float *grad_view, const void *left, float *grad_prob, void *stream);

/* Semi-global matching (Hirschmueller, TPAMI 2008) with a census cost: a second matcher beside the engine, engine-free.
 * The rule is integer up to one float32 division, so every implementation gives the same bits.
 *   - Input: n pairs of planar [C][H][W] frames, C in {1, 3}, SMX_DTYPE_U8 or SMX_DTYPE_F32.  Candidate i in 0..D-1
 *     (D = num_disparities, 1..256) means disparity dmin + i (dmin = min_disparity, 0..32768): the left pixel (y, x)
 *     matches the right pixel (y, x - dmin - i).
 *   - Gray: for C = 3, (0.2989f*r + 0.5870f*g) + 0.1140f*b in float32 with no contraction (the engine's step 1, on the
 *     values or on float(u8)); for C = 1, the values themselves.
 *   - Census: a 9 wide x 7 high window; bit k is set when the k-th of its 62 neighbours (row-major, centre skipped) is
 *     < the centre under IEEE < (a NaN gives 0).  Neighbour coordinates are clamped into the image.
 *   - Cost: C(p, i) = popcount(cL(y, x) ^ cR(y, x - dmin - i)), and 64 when x - dmin - i < 0.
 *   - Paths: 4, the directions (0,+1), (0,-1), (+1,0), (-1,0), or 8, which add the four diagonals.  With q = p - r the
 *     predecessor of p on path r: L_r(p,i) = C(p,i) when q lies outside the image, otherwise
 *       L_r(p,i) = C(p,i) + min(L_r(q,i), L_r(q,i-1) + P1, L_r(q,i+1) + P1, M_r(q) + P2) - M_r(q),
 *     M_r(q) = min_k L_r(q,k); a neighbour i+-1 outside 0..D-1 is left out of the min.  0 <= P1 <= P2 <= 191, so
 *     L_r <= 255 and S = sum_r L_r <= 2040.
 *   - Winner: i* is the smallest i minimising S(p, i); d* = dmin + i*.
 *   - Invalid (the pixel is invalid_disparity): (a) x - d* < 0; (b) uniqueness u in 1..99 (0: off) and some i with
 *     |i - i*| > 1 has S(i) * (100 - u) < S(i*) * 100; (c) lr_max_diff >= 0 and |dmin + iR(y, x - d*) - d*| >
 *     lr_max_diff, where iR(y, x') is the smallest i minimising S(y, x' + dmin + i, i) over the i with
 *     x' + dmin + i <= W - 1 (the right-view winner, from the same S).  A negative lr_max_diff turns (c) off.
 *   - Value: with subpixel != 0 and 0 < i* < D-1, den = S(i*-1) + S(i*+1) - 2 S(i*); if den > 0 the output is
 *     f32(d*) + f32(S(i*-1) - S(i*+1)) / f32(2 den) (one correctly rounded division, then one add), else f32(d*).
 *   - gray_left_out (NULL: not written): the f32 [n][H][W] gray planes of the left frames, the weighted median's guide.
 * left / right: [n][C][H][W] device frames; out: [n][H][W] f32.  out and gray_left_out must not overlap an input, the
 * workspace or each other.  workspace: device memory of at least smx_sgm_workspace_bytes(n, H, W, D, paths) bytes; its
 * contents on entry do not matter.  With P = n*H*W, Dp = D rounded up to a multiple of (D <= 64 ? 1 : D <= 128 ? 2 : 4)
 * and R(v) = v rounded up to a multiple of 256, the size is
 *     R(8 P) + R(8 P) + R(2 Dp P) + R(2 P)
 * (two census planes, the u16 volume S and the right-view winners; the same for 4 and 8 paths).  It is 0 for
 * arguments smx_sgm would reject by size.  A batch whose n * (H + W) exceeds 2^31 must be split by the caller.
 * A fixed sequence of 4 to 7 launches on `stream` (a caller's stream), with no host synchronisation and no allocation,
 * so it can be captured into a HIP graph.  Engine-free: device_id only selects the device.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL left, right, out or workspace, n < 1, H or W
 * outside 1..32768, n * (H + W) > 2^31, channels not 1 or 3, an unknown dtype, min_disparity outside 0..32768,
 * num_disparities outside 1..256, paths not 4 or 8, not 0 <= P1 <= P2 <= 191, uniqueness outside 0..99, a non-finite
 * lr_max_diff or invalid_disparity, workspace_bytes below the query, the overlaps above, stream == SMX_STREAM_ENGINE. */
size_t smx_sgm_workspace_bytes(int n, int H, int W, int num_disparities, int paths);
int smx_sgm(int device_id, int n, int channels, int dtype, int H, int W, const void *left, const void *right,
            int min_disparity, int num_disparities, int paths, int P1, int P2, int uniqueness, float lr_max_diff,
            int subpixel, float invalid_disparity, float *out, float *gray_left_out, void *workspace,
            size_t workspace_bytes, void *stream);
/* smx_sgm that also writes the right-view map: right_out ([n][H][W] f32, required) receives f32(dmin + iR(y, x')) where
 * iR >= 0 and invalid_disparity where no candidate lies in the image (iR = -1), iR as above, whether or not lr_max_diff
 * is negative (the right-view winners are then found for this map alone).  out and gray_left_out are the same bits as
 * smx_sgm's for the same arguments, and the workspace query is the same.  right_out must not overlap an input, the
 * workspace, out or gray_left_out.  The other arguments and their checks are smx_sgm's; a NULL right_out is
 * SMX_ERR_INVALID_ARG. */
int smx_sgm_with_right_map(int device_id, int n, int channels, int dtype, int H, int W, const void *left,
                           const void *right, int min_disparity, int num_disparities, int paths, int P1, int P2,
                           int uniqueness, float lr_max_diff, int subpixel, float invalid_disparity, float *out,
                           float *gray_left_out, float *right_out, void *workspace, size_t workspace_bytes,
                           void *stream);

/* ---- Metric 3D point clouds -------------------------------------------------------------------------------------------
 * smx_reproject_points: n disparity maps disp [n][H][W] f32 -> one compacted list of 3D points for the batch.
 * Geometry: Q is a host 4x4 row-major matrix in OpenCV's reprojectImageTo3D convention, [X' Y' Z' W'] = Q [u v d 1], with
 * u = (float)column and v = (float)row.  Every step is ONE float32 operation (no fused multiply-add, correctly rounded
 * division), in this order, on every implementation:
 *   R'   = ((Q[r][0]*u + Q[r][1]*v) + Q[r][2]*d) + Q[r][3]          for r = 0..3  (X', Y', Z', W')
 *   X = X'/W', Y = Y'/W', Z = Z'/W'
 * A pixel becomes a point iff d is finite and d != invalid_disparity, W' > 0, X, Y and Z are finite,
 * z_min <= Z <= z_max, and (with a confidence map) c >= min_confidence (a NaN c excludes the pixel).
 * Colour (image != NULL): gray [n][H][W] (image_channels 1, copied to R, G and B) or planar RGB [n][3][H][W]
 * (image_channels 3), SMX_DTYPE_U8 or SMX_DTYPE_F32; an f32 value v becomes (uint8)clamp(floorf(v + 0.5f), 0, 255),
 * NaN -> 0.
 * Outputs (capacity n*H*W points; the caller allocates it): offsets [n+1] int32 on the device -- the points of map i are
 * [offsets[i], offsets[i+1]), in row-major pixel order; points [cap][3] f32; colors [cap][3] u8 (NULL: none; needs an
 * image); indices [cap] int32 (NULL: none), the pixel's row-major index y*W + x within its map; xyz_map
 * [n][H][W][3] f32 (NULL: none), the organised cloud with NaN at every excluded pixel.  Entries past offsets[n] are not
 * written.  workspace: smx_reproject_workspace_bytes(n, H, W) bytes (0 for sizes the call rejects).
 * Three launches on `stream` (a caller's stream), no host synchronisation and no allocation: graph-capturable.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL disp, Q, points, offsets or workspace; n < 1; H or W
 * outside 1..32768; n*H*W > 2^30; a non-finite Q entry; a NaN z bound or z_min > z_max; a non-finite min_confidence or
 * invalid_disparity; an image whose channels are not 1 or 3 or whose dtype is unknown; colors without an image;
 * workspace_bytes below the query; an output overlapping an input, the workspace or another output; stream ==
 * SMX_STREAM_ENGINE. */
size_t smx_reproject_workspace_bytes(int n, int H, int W);
int smx_reproject_points(int device_id, int n, int H, int W, const float *disp, const float Q[16],
                         const float *confidence, float min_confidence, float z_min, float z_max,
                         float invalid_disparity, const void *image, int image_channels, int image_dtype,
                         float *points, uint8_t *colors, int32_t *indices, float *xyz_map, int32_t *offsets,
                         void *workspace, size_t workspace_bytes, void *stream);

/* smx_voxel_downsample: one point per occupied voxel of every map of a compacted list (smx_reproject_points' output:
 * points [capacity][3] f32, colors [capacity][3] u8 or NULL, offsets [n+1] int32 on the device).  The device offsets are
 * used clamped to a non-decreasing sequence in [0, capacity].
 *   voxel index per axis: i = (int)floorf(coord / voxel_size); a point with any index outside -2^20 <= i < 2^20 (or a
 *   NaN coordinate) is dropped and counted in dropped[map].
 *   A voxel with cnt < min_points points is dropped and its cnt points are counted in dropped[map].
 *   Per map, the kept voxels are written in ascending (ix, iy, iz) order from out_offsets[map]:
 *     centroid  = S / (float)cnt per axis, S summed over the voxel's points in their input (pixel) order: sequentially
 *                 within consecutive chunks of 64 points, s_c = ((p_0 + p_1) + p_2) + ... (starting from p_0, not
 *                 0), then sequentially over the chunk sums, S = ((s_0 + s_1) + s_2) + ...; one point returns itself.
 *     colour    = (sum of c + cnt/2) / cnt per channel, in integers (out_colors; only with colors)
 *     out_counts = cnt
 *   out_offsets [n+1] int32, dropped [n] int32; the sum of out_counts of map i plus dropped[i] is its input count.
 * The result is bit-identical from run to run, and map i's is independent of n and of the other maps: there are no
 * float atomics (a stable LSD radix sort of each map's voxel keys, then one thread per voxel).
 * workspace: smx_voxel_workspace_bytes(n, capacity) bytes (0 for sizes the call rejects); about 36 bytes per point.
 * A fixed sequence of launches on `stream` (a caller's stream; sort passes beyond the key's width return at once), no host
 * synchronisation and no allocation: graph-capturable.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL points, offsets, out_points, out_counts,
 * out_offsets, dropped or workspace; exactly one of colors / out_colors NULL; n outside 1..65536; capacity outside
 * 1..2^30; voxel_size not finite and > 0; min_points < 1; workspace_bytes below the query; an output overlapping an input,
 * the workspace or another output; stream == SMX_STREAM_ENGINE. */
size_t smx_voxel_workspace_bytes(int n, int capacity);
int smx_voxel_downsample(int device_id, int n, int capacity, const float *points, const uint8_t *colors,
                         const int32_t *offsets, float voxel_size, int min_points, float *out_points,
                         uint8_t *out_colors, int32_t *out_counts, int32_t *out_offsets, int32_t *dropped,
                         void *workspace, size_t workspace_bytes, void *stream);

/* smx_project_points: the inverse of smx_reproject_points -- n point clouds projected into n camera views of H x W
 * pixels as disparity maps, with a depth test.  points [capacity][3] f32 and offsets [n+1] int32 on the device: cloud f
 * is rows [offsets[f], offsets[f+1]), the offsets used clamped to a non-decreasing sequence in [0, capacity] as
 * smx_voxel_downsample uses them; point j of a cloud is its j-th row.  world_to_camera [n][3][4] f32 (device, row-major),
 * as for smx_tsdf_integrate; P: host 4x4, [u' v' d' w'] = P [X Y Z 1] (the Python layer passes inv(Q), computed in float64
 * and rounded once).  radius in 0..8: a point covers the square of (2 radius + 1)^2 pixels around its pixel.
 * Every step is ONE float32 operation (no fused multiply-add, correctly rounded division), in this order, on every
 * implementation.  For point j = (x, y, z) of cloud f, with M = world_to_camera[f]:
 *   c_r = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3]            r = 0, 1, 2
 *   skip unless c_2 is finite, c_2 > 0 and z_min <= c_2 <= z_max
 *   p_r = ((P[r][0]*c_0 + P[r][1]*c_1) + P[r][2]*c_2) + P[r][3]      r = 0, 1, 2, 3
 *   skip unless p_3 > 0
 *   fu = floorf(p_0/p_3 + 0.5f), fv = floorf(p_1/p_3 + 0.5f)
 *   skip unless -R <= fu <= (W-1)+R and -R <= fv <= (H-1)+R          R = (float)radius; compared as floats, NaN fails
 *   d = p_2/p_3; skip unless d is finite and d != invalid_disparity
 *   the point is a candidate for every pixel ((int)fu + dx, (int)fv + dy), |dx|, |dy| <= radius, that lies in the image
 * The winner of a pixel is its candidate with the smallest c_2 and, among equal c_2, the smallest j: c_2 > 0, so its bit
 * pattern orders as an unsigned integer, and the winner is the minimum of the 64-bit keys (bits(c_2) << 32) | j.
 * Outputs: disp [n][H][W] f32, the winner's d, invalid_disparity where no point lands; index [n][H][W] int32 (NULL: none),
 * the winner's j, -1 where none; depth [n][H][W] f32 (NULL: none), the winner's c_2, NaN where none.  The result depends
 * on neither the grid, the scheduling nor n: cloud f's view is the same bits alone or in a batch, and from run to run.
 * Three launches on `stream` (a caller's stream) -- clear the keys, splat, resolve -- with integer atomics only (one
 * 64-bit unsigned minimum per candidate), no float atomics, no host synchronisation and no allocation: graph-capturable.
 * workspace: smx_project_workspace_bytes(n, H, W) bytes -- the keys, 8 bytes per output pixel, and the n+1 clamped
 * offsets, each rounded up to 256 bytes; 0 for sizes the call rejects.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL points, offsets, world_to_camera, P, disp or
 * workspace; n outside 1..65536; capacity outside 1..2^30; H or W outside 1..32768 or n*H*W > 2^30; radius outside 0..8;
 * a non-finite P entry; a NaN z bound or z_min > z_max; a non-finite invalid_disparity; workspace_bytes below the query;
 * an output or the workspace overlapping an input or another output; stream == SMX_STREAM_ENGINE. */
size_t smx_project_workspace_bytes(int n, int H, int W);
int smx_project_points(int device_id, int n, int capacity, int H, int W, const float *points, const int32_t *offsets,
                       const float *world_to_camera, const float P[16], int radius, float z_min, float z_max,
                       float invalid_disparity, float *disp, int32_t *index, float *depth, void *workspace,
                       size_t workspace_bytes, void *stream);

/* ---- TSDF fusion ----------------------------------------------------------------------------------------------------
 * A volume of nx * ny * nz voxels with edge s = voxel_size and origin o (host float[3]); voxel (i, j, k) has the linear
 * index (k*ny + j)*nx + i and the centre g = (o_x + ((float)i + 0.5f)*s, o_y + ((float)j + 0.5f)*s,
 * o_z + ((float)k + 0.5f)*s).  Its state is caller-owned device memory: tsdf [nz][ny][nx] f32, weight [nz][ny][nx] f32
 * and, optionally, color [nz][ny][nx][4] u8 (R, G, B, 0: one aligned 32-bit word per voxel).  The empty state is all
 * zero.  The camera frame is smx_reproject_points': x right, y down, z forward; the world frame is the caller's.
 * Every step below is ONE float32 operation (no fused multiply-add, correctly rounded division and sqrtf), in the stated
 * order, on every implementation.
 *
 * smx_tsdf_integrate: n maps disp [n][H][W] f32 with their poses world_to_camera [n][3][4] f32 (device, row-major),
 * applied in order.  Q: host 4x4, as for smx_reproject_points; P: host 4x4, the projection [u' v' d' w'] = P [X Y Z 1]
 * (the Python layer sets P = inv(Q), computed in float64 and rounded once to float32).
 *   Pixel (px, py) of map f, u = (float)px, v = (float)py, d = disp[f][py][px], is accepted iff d is finite and
 *   d != invalid_disparity; W' = ((Q30*u + Q31*v) + Q32*d) + Q33 > 0; Zm = Z'/W' is finite, with
 *   Z' = ((Q20*u + Q21*v) + Q22*d) + Q23; z_min <= Zm <= z_max; and, with a confidence map, c >= min_confidence and
 *   c > 0 (a NaN c excludes the pixel).  Its weight w is c, or 1.0f without a confidence map; its colour I is the
 *   image's (gray [n][H][W] copied to R, G and B, or planar RGB [n][3][H][W]; u8, or f32 v ->
 *   (uint8)clamp(floorf(v + 0.5f), 0, 255) with NaN -> 0), as a float per channel.
 *   For each voxel, for f = 0 .. n-1 in order, with M = world_to_camera[f]:
 *     c_r = ((M[r][0]*g_x + M[r][1]*g_y) + M[r][2]*g_z) + M[r][3]          r = 0, 1, 2
 *     skip unless c_2 > 0
 *     p_r = ((P[r][0]*c_0 + P[r][1]*c_1) + P[r][2]*c_2) + P[r][3]          r = 0, 1, 3
 *     skip unless p_3 > 0
 *     fu = floorf(p_0/p_3 + 0.5f), fv = floorf(p_1/p_3 + 0.5f)
 *     skip unless 0 <= fu <= W-1 and 0 <= fv <= H-1 (compared as floats; NaN fails)
 *     skip unless pixel ((int)fu, (int)fv) of map f is accepted
 *     sdf = Zm - c_2; skip unless sdf >= -truncation
 *     t = fminf(sdf / truncation, 1.0f)
 *     T = ((T0*W0) + (t*w)) / (W0 + w);  W = fminf(W0 + w, max_weight)
 *     C = ((C0*W0) + (I*w)) / (W0 + w) per channel, stored as (uint8)floorf(C + 0.5f) (C lies in [0, 255] for a finite
 *         w; a NaN C, from an infinite confidence, stores 0), with a zero fourth byte
 *   where T0, W0 and C0 are the voxel's values before the frame; frame f's result is frame f+1's input.  Hence a voxel
 *   that no frame of the call measures is not written, and one call with n maps gives the same bits as n calls with
 *   one map each.
 * Two launches on `stream` (a caller's stream), no atomics, no host synchronisation and no allocation:
 * graph-capturable.  workspace: smx_tsdf_integrate_workspace_bytes(n, H, W) bytes (12 per pixel; 0 for sizes the call
 * rejects).
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL origin, tsdf, weight, disp, Q, P, world_to_camera or
 * workspace; nx, ny or nz outside 1..4096 or nx*ny*nz > 2^30; n < 1, H or W outside 1..32768 or n*H*W > 2^30;
 * voxel_size not finite and > 0; truncation not finite or <= voxel_size; max_weight not finite and > 0; a non-finite Q,
 * P or origin entry; a NaN z bound or z_min > z_max; a non-finite min_confidence or invalid_disparity; color without an
 * image; an image whose channels are not 1 or 3 or whose dtype is unknown; workspace_bytes below the query; a state
 * array or the workspace overlapping an input or each other; stream == SMX_STREAM_ENGINE. */
size_t smx_tsdf_integrate_workspace_bytes(int n, int H, int W);
int smx_tsdf_integrate(int device_id, int nx, int ny, int nz, const float origin[3], float voxel_size,
                       float truncation, float max_weight, float *tsdf, float *weight, uint8_t *color, int n, int H,
                       int W, const float *disp, const float Q[16], const float P[16], const float *world_to_camera,
                       const float *confidence, float min_confidence, float z_min, float z_max,
                       float invalid_disparity, const void *image, int image_channels, int image_dtype,
                       void *workspace, size_t workspace_bytes, void *stream);

/* smx_tsdf_extract_points: the zero crossings of a volume (smx_tsdf_integrate's state) as points.  Voxels are visited in
 * ascending linear index and each voxel's axes in the order x, y, z.  For axis a and the neighbour v' = v + e_a inside
 * the grid, a point is emitted iff weight[v] >= min_weight and weight[v'] >= min_weight, (T0 >= 0) != (T1 >= 0), and
 * |T0| < 1 and |T1| < 1 (T0 = tsdf[v], T1 = tsdf[v']; the last condition rejects the false crossings between truncated
 * free space and the space behind a surface at occlusion edges).  For an emitted point:
 *   position  t = T0 / (T0 - T1); the point is g(v) with its a coordinate replaced by g_a(v) + t*s
 *   normal    (normals != NULL) the central differences x_b = T[v+e_b] - T[v-e_b] for b = x, y, z, with indices clamped
 *             to the grid, each divided by len = sqrtf((x_x*x_x + x_y*x_y) + x_z*x_z); len == 0 gives (0, 0, 0).  It
 *             points toward positive T, i.e. toward the cameras.
 *   colour    (colors != NULL; needs color) the R, G, B of v if t <= 0.5f, else those of v'
 * Outputs: count (device int32) = the total number of crossings (saturated at 2^31 - 1); the first min(total, capacity)
 * points in the order above to points [capacity][3] f32, normals [capacity][3] f32 and colors [capacity][3] u8; nothing
 * past them is written.  Three steps on `stream` (a caller's stream): count per (k, j) row, an exclusive scan of the
 * row counts, ordered scatter per row; no atomics, no host synchronisation, no allocation: graph-capturable.
 * workspace: smx_tsdf_extract_workspace_bytes(nx, ny, nz) bytes (about 8 per row of x voxels; 0 for sizes the call
 * rejects).
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL origin, tsdf, weight, points, count or workspace;
 * the volume's dimension, voxel_size and origin checks of smx_tsdf_integrate; min_weight not finite and > 0; capacity
 * outside 1..2^30; colors without color; workspace_bytes below the query; an output or the workspace overlapping an
 * input or another output; stream == SMX_STREAM_ENGINE. */
size_t smx_tsdf_extract_workspace_bytes(int nx, int ny, int nz);
int smx_tsdf_extract_points(int device_id, int nx, int ny, int nz, const float origin[3], float voxel_size,
                            const float *tsdf, const float *weight, const uint8_t *color, float min_weight,
                            int capacity, float *points, float *normals, uint8_t *colors, int32_t *count,
                            void *workspace, size_t workspace_bytes, void *stream);

/* smx_tsdf_extract_triangles: the surface of a volume as an indexed triangle mesh whose vertices are, by index, the
 * points smx_tsdf_extract_points emits for the same min_weight (marching cubes; this call writes the connectivity only).
 * A cell (i, j, k) exists for 0 <= i < nx-1, 0 <= j < ny-1, 0 <= k < nz-1; its corner c = cx + 2*cy + 4*cz is the voxel
 * (i+cx, j+cy, k+cz).  A cell is VALID iff all eight corners have weight >= min_weight and |T| < 1; a corner is inside
 * iff T < 0, and the cell's case is the sum of 2^c over its inside corners.  Cells are visited in ascending linear index
 * (k*ny + j)*nx + i; a valid cell emits the triangles of its case in table order, three int32 vertex indices each; other
 * cells emit nothing.
 *   edges     e = 4*a + r runs along axis a (x 0, y 1, z 2) from a base corner b whose offset along a is 0, with r
 *             x: cy + 2*cz, y: cx + 2*cz, z: cx + 2*cy of b.  The vertex of edge e of cell (i, j, k) is the crossing of
 *             voxel (i, j, k) + b along a; every crossed edge of a valid cell satisfies smx_tsdf_extract_points' emission
 *             rule, and the vertex index is the rank of that (voxel, axis) crossing in that call's output order.
 *   table     per face of the cell: with 0 or 4 inside corners nothing; otherwise one segment joins the face's two
 *             crossed edges; with two diagonally opposite inside corners two segments, each joining the two edges that
 *             meet at an inside corner.  A face's segments depend on its four signs only, so neighbouring cells agree and
 *             the mesh is closed wherever the cells around it are valid.  The segments of a case form closed loops; each
 *             loop starts at its lowest edge id and is fanned from there, (l0, l_m, l_m+1), loops in the order of their
 *             lowest edge id; at most 5 triangles.  For every triangle (a, b, c), (b - a) x (c - a) points from inside
 *             (T < 0) to outside (T >= 0, where the cameras are): the side the vertex normals point to.
 *             cuda_depth/mc_table.py generates the table from this rule.
 * Crossings that no valid cell touches stay in the vertex list as unreferenced vertices: indices are not compacted.
 * Outputs: count (device int32) = the total number of triangles (saturated at 2^31 - 1); the first min(total, capacity)
 * triangles to triangles [capacity][3] int32; nothing past them is written.  A volume with more than 2^31 - 1 crossings
 * has vertices that an int32 cannot index: count = -1 and nothing is written (decided on the device).  On `stream` (a
 * caller's stream): one pass over the volume, counts per (k, j) row, one exclusive scan, ordered scatter per row; no
 * atomics, no host synchronisation, no allocation: graph-capturable and deterministic.
 * workspace: smx_tsdf_extract_triangles_workspace_bytes(nx, ny, nz) bytes (one per voxel, 4 per 64 voxels of a row and
 * about 24 per row; 0 for sizes the call rejects).
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL tsdf, weight, triangles, count or workspace; the
 * volume's dimension checks of smx_tsdf_integrate; min_weight not finite and > 0; capacity outside 1..2^30;
 * workspace_bytes below the query; an output or the workspace overlapping an input or another output;
 * stream == SMX_STREAM_ENGINE. */
size_t smx_tsdf_extract_triangles_workspace_bytes(int nx, int ny, int nz);
int smx_tsdf_extract_triangles(int device_id, int nx, int ny, int nz, const float *tsdf, const float *weight,
                               float min_weight, int capacity, int32_t *triangles, int32_t *count, void *workspace,
                               size_t workspace_bytes, void *stream);

/* smx_tsdf_raycast: n views of a volume (smx_tsdf_integrate's state, read only) by ray casting, one ray per pixel.
 * camera_to_world [n][3][4] f32 (device, row-major): the pose of each view (not inverted); Q: host 4x4, shared by the
 * views, whose ray must not depend on d: Q02 = Q12 = Q22 = 0, Q30 = Q31 = 0, Q32 != 0 (what reprojection_matrix builds).
 *   ray       pixel (px, py) of view f, u = (float)px, v = (float)py, M = camera_to_world[f]:
 *               X' = (Q00*u + Q01*v) + Q03,  Y' = (Q10*u + Q11*v) + Q13,  Z' = (Q20*u + Q21*v) + Q23
 *               no ray (hence no hit) unless Z' > 0;  rx = X'/Z', ry = Y'/Z'
 *               dw_r = (M[r][0]*rx + M[r][1]*ry) + M[r][2],  e_r = M[r][3]          r = 0, 1, 2
 *             The ray parameter lam is camera depth: the point at lam is p_a = e_a + dw_a*lam.
 *   Tri(p)    the volume at a point p: g_a = (p_a - o_a)/s - 0.5f, f_a = floorf(g_a); p is IN BOUNDS iff
 *             0 <= f_a <= n_a - 2 on every axis (compared as floats; NaN fails); then, with the corners
 *             c(cx, cy, cz) = tsdf of voxel (f_x + cx, f_y + cy, f_z + cz), the fractions t_a = g_a - f_a and
 *             lerp(a, b, t) = a + (b - a)*t:  along x  c_yz = lerp(c(0, y, z), c(1, y, z), t_x),  then y
 *             c_z = lerp(c_0z, c_1z, t_y),  then z  Tri = lerp(c_0, c_1, t_z).
 *   samples   lam_m = z_min + (float)m*step for m = 0 .. M-1, M = (int)floorf((z_max - z_min)/step) + 1 (float32
 *             subtraction, division and floorf).  Every lam_m is computed from m, never accumulated.  Sample m, at the
 *             point of lam_m, is VALID iff that point is in bounds and its eight corners have weight >= min_weight; its
 *             value is T_m = Tri there.
 *   hit       the first m whose sample is valid with T_m < 0 ends the ray; invalid samples are walked through.  The ray
 *             hits iff sample m-1 exists, is valid and 0 <= T_{m-1} < 1 (a ray that starts behind a surface, and the
 *             jump from truncated free space to the space behind a surface at an occlusion edge -- the reason
 *             smx_tsdf_extract_points asks for |T| < 1 -- do not); a ray that no sample ends does not hit.  On a hit
 *               lam* = lam_{m-1} + step*(T_{m-1}/(T_{m-1} - T_m)),  p*_a = e_a + dw_a*lam*
 * Outputs, planes [n][H][W]; disp is required, each other output may be NULL and is then not written:
 *   disp      f32  (Z'/lam* - Q33)/Q32, or invalid_disparity without a hit: the convention of every [H, W] map entry
 *   depth     f32  lam*, or NaN without a hit
 *   normals   [n][3][H][W] f32, world frame, toward positive T: x_a = Tri(p* with p*_a + s in place of p*_a) -
 *             Tri(p* with p*_a - s in place of p*_a) for a = x, y, z (the corners' weights are not tested, as in
 *             smx_tsdf_extract_points), each divided by len = sqrtf((x_x*x_x + x_y*x_y) + x_z*x_z); (0, 0, 0) where one
 *             of the six probes is not in bounds, where len == 0, and without a hit
 *   colors    [n][3][H][W] u8 (needs color): R, G, B of the voxel nearest to p*, index
 *             fminf(fmaxf(floorf(g_a + 0.5f), 0.0f), (float)(n_a - 1)) per axis with g of p*; 0 without a hit
 *   weight    f32  that voxel's weight, or 0 without a hit
 * Three launches on `stream` (a caller's stream), no atomics, no host synchronisation, no allocation: graph-capturable.
 * The first two write one byte per brick of 8 x 8 x 8 voxels to the workspace: whether a voxel of the brick has weight >=
 * min_weight, and whether every voxel that a cell with its first corner in the brick can touch has weight >= min_weight
 * and tsdf == 1.0f exactly (measured free space, where a sample is valid with T = 1 exactly: every lerp is
 * 1 + (1 - 1)*t).  The third marches one thread per pixel and jumps over runs of samples that lie outside the volume's
 * box, whose first corner lies in an empty brick (invalid by the rule above) or in a free one (valid with T = 1: none
 * ends the ray).  The result is the rule's, bit for bit, whatever is jumped over.
 * workspace: smx_tsdf_raycast_workspace_bytes(nx, ny, nz) bytes (two per brick; 0 for sizes the call rejects).
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL origin, tsdf, weight, Q, camera_to_world, disp or
 * workspace; the volume's dimension, voxel_size and origin checks of smx_tsdf_integrate; n < 1, H or W outside 1..32768
 * or n*H*W > 2^30; min_weight not finite and > 0; step not finite and > 0; z_min or z_max not finite, z_min < 0 or
 * z_min > z_max; M outside 1..65536; a non-finite Q entry or a Q outside the accepted form; a non-finite
 * invalid_disparity; colors without color; workspace_bytes below the query; an output or the workspace overlapping an
 * input or another output; stream == SMX_STREAM_ENGINE. */
size_t smx_tsdf_raycast_workspace_bytes(int nx, int ny, int nz);
int smx_tsdf_raycast(int device_id, int nx, int ny, int nz, const float origin[3], float voxel_size,
                     const float *tsdf, const float *weight, const uint8_t *color, float min_weight, int n, int H,
                     int W, const float Q[16], const float *camera_to_world, float step, float z_min, float z_max,
                     float invalid_disparity, float *disp, float *depth, float *normals, uint8_t *colors,
                     float *out_weight, void *workspace, size_t workspace_bytes, void *stream);

/* smx_tsdf_window: a window of a volume's state as the state of a volume of its own -- what moves a volume with the
 * camera in whole-voxel steps (the same dims, the start = the shift), crops or grows it, and cuts out the slab a shift
 * leaves behind.  The source is smx_tsdf_integrate's state of nx * ny * nz voxels, read only; the window starts at source
 * voxel (x0, y0, z0), of any sign, and has bx * by * bz voxels: the dims of the destination arrays tsdf_out, weight_out
 * [bz][by][bx] f32 and color_out [bz][by][bx][4] u8.  It may lie partly or wholly outside the source.
 *   For every destination voxel (i, j, k), 0 <= i < bx, 0 <= j < by, 0 <= k < bz, the source voxel is
 *   (x0 + i, y0 + j, z0 + k).  If 0 <= x0 + i < nx, 0 <= y0 + j < ny and 0 <= z0 + k < nz, the destination's three state
 *   words are the source voxel's, copied bit for bit (NaN payloads and -0.0f are kept and the colour word is whole: no
 *   float operation touches a value); otherwise all three are the empty state, all-zero bits.
 * The destination describes the same world when its origin is the source's moved by (x0, y0, z0) voxels: the caller's
 * arithmetic (the Python layer keeps the first origin and an integer offset, and multiplies once, in float64).
 * A shift by (dx, dy, dz) is the window (dx, dy, dz) at the volume's own dims, written to a second set of arrays that
 * then becomes the state: a volume that shifts needs twice its state's memory while that spare set exists.  What a
 * shift leaves behind is cut out BEFORE it, as one box per axis with a non-zero component: the whole cross-section in
 * the other two axes and, along its own axis a with n = n_a and d = d_a, the layers [0, min(n, d + margin)) for d > 0 or
 * [max(0, n + d - margin), n) for d < 0 -- the leaving layers plus `margin` layers of the staying side, so that with
 * margin >= 1 a crossing between a leaving voxel and a staying one is in a box.  Surface elements wholly inside a margin
 * layer then exist twice, in the box and in the shifted volume, and so do those in the corner two boxes share;
 * smx_voxel_downsample at voxel_size removes the duplicates from point clouds.  Boxes are ordinary volumes for every
 * entry above, and smx_tsdf_merge in FILL mode writes a box back when the volume returns to the place it left (the Python
 * layer's TSDFSpillStore keeps the boxes and does so).  Not addressed: loop closure and relocalisation.
 * color and color_out are both NULL or both given.  The call is out of place: a destination array may overlap neither a
 * source array nor another destination array.
 * One launch on `stream` (a caller's stream), no atomics, no workspace, no host synchronisation and no allocation:
 * graph-capturable.
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL tsdf, weight, tsdf_out or weight_out; color without
 * color_out or color_out without color; nx, ny, nz or bx, by, bz outside 1..4096 or a product > 2^30; |x0|, |y0| or |z0|
 * > 8192; a destination array overlapping a source array or another destination array; stream == SMX_STREAM_ENGINE. */
int smx_tsdf_window(int device_id, int nx, int ny, int nz, const float *tsdf, const float *weight, const uint8_t *color,
                    int x0, int y0, int z0, int bx, int by, int bz, float *tsdf_out, float *weight_out,
                    uint8_t *color_out, void *stream);

/* smx_tsdf_merge: one volume's state written into another -- what restores a spilled box when a volume returns to a place
 * it left, and what joins two volumes fused from different frames.  The destination is smx_tsdf_integrate's state of
 * nx * ny * nz voxels, tsdf, weight [nz][ny][nx] f32 and color [nz][ny][nx][4] u8, updated IN PLACE.  The source is a state
 * of sx * sy * sz voxels, src_tsdf, src_weight [sz][sy][sx] and src_color, read only.  Source voxel (0, 0, 0) sits at
 * destination voxel (x0, y0, z0), of any sign.  Only the REGION of the source that starts at source voxel (rx, ry, rz)
 * and has cx * cy * cz voxels takes part: source voxel s of the region pairs with destination voxel d = s + (x0, y0, z0),
 * and pairs whose d lies outside the destination grid are ignored.  A region with no pair launches nothing and returns 0.
 *   Every step is ONE float32 operation (no fused multiply-add, correctly rounded division).  For a pair, T1, W1, C1 are
 *   the source's tsdf, weight and colour, T0, W0, C0 the destination's:
 *     skip unless W1 > 0.0f (a NaN fails the test; the destination's bits stay as they are)
 *     if not W0 > 0.0f: the destination's three words become the source's, copied bit for bit (NaN payloads and -0.0f
 *       are kept and the colour word is whole, fourth byte included: no float operation touches a value)
 *     else with mode == SMX_TSDF_MERGE_FILL: the destination stays as it is
 *     else with mode == SMX_TSDF_MERGE_AVERAGE, smx_tsdf_integrate's form with the source as the measurement:
 *       T = ((T0*W0) + (T1*W1)) / (W0 + W1);  W = fminf(W0 + W1, max_weight)
 *       C = ((C0*W0) + (C1*W1)) / (W0 + W1) per channel, stored as (uint8)floorf(C + 0.5f) (C lies in [0, 255] for
 *           finite weights; a NaN C stores 0), with a zero fourth byte
 *   With finite tsdf values and weights that is all; the payloads of NaNs that the AVERAGE arithmetic produces from
 *   non-finite values are not pinned.
 * FILL gives back what a shift cut out: the box's voxels go where the volume holds nothing, and what the volume has
 * measured since wins.  AVERAGE of two volumes fused from disjoint frames equals, up to rounding, one volume fused from
 * all of them as long as no weight reaches max_weight (a weighted mean is associative; the cap is not).
 * color and src_color are both NULL or both given.  A destination array may overlap neither a source array nor another
 * destination array: a volume is not merged into itself.
 * One launch on `stream` (a caller's stream), no atomics, no workspace, no host synchronisation and no allocation:
 * graph-capturable.  Every destination voxel has one owner thread, so the update in place is safe.
 * SMX_ERR_INVALID_ARG, checked before the device is touched, in this order: a NULL tsdf, weight, src_tsdf or src_weight;
 * color without src_color or src_color without color; nx, ny, nz outside 1..4096 or a product > 2^30; the same for sx,
 * sy, sz; |x0|, |y0| or |z0| > 8192; a region that is not inside the source (rx, ry, rz < 0, cx, cy, cz < 1,
 * rx + cx > sx, ry + cy > sy or rz + cz > sz); a mode other than the two; max_weight not finite and > 0 (in both modes);
 * a destination array overlapping a source array or another destination array; stream == SMX_STREAM_ENGINE. */
#define SMX_TSDF_MERGE_FILL    0
#define SMX_TSDF_MERGE_AVERAGE 1
int smx_tsdf_merge(int device_id, int nx, int ny, int nz, float *tsdf, float *weight, uint8_t *color,
                   int sx, int sy, int sz, const float *src_tsdf, const float *src_weight, const uint8_t *src_color,
                   int x0, int y0, int z0, int rx, int ry, int rz, int cx, int cy, int cz,
                   int mode, float max_weight, void *stream);

/* ---- Camera tracking -------------------------------------------------------------------------------------------------
 * smx_track_camera: the camera-to-world pose of a frame from its disparity map, by projective point-to-plane ICP against
 * a rendered view of the model (KinectFusion's frame-to-model tracking).  It handles n independent triples (frame, model
 * view, initial pose).  Every step below is ONE float32 operation (no fused multiply-add, correctly rounded division and
 * sqrtf) unless it is stated as float64; float64 steps are single operations as well.
 *   frame     disp [n][H][W] f32, optional confidence [n][H][W], Q (host 4x4).  Pixel (px, py) of frame f is ACCEPTED iff
 *             smx_tsdf_integrate's pixel rule accepts it (d finite and != invalid_disparity, W' > 0, Zm finite in
 *             [z_min, z_max], c >= min_confidence and c > 0) and its camera point (X, Y, Z) = (X'/W', Y'/W', Z'/W') of
 *             smx_reproject_points is finite; its weight w is c, or 1.0f without a confidence map.  An iteration of stride
 *             s SELECTS the pixels with px % s == 0 and py % s == 0: the selected grid has Ws = ceil(W/s) columns and
 *             Hs = ceil(H/s) rows, selected pixel (sx, sy) being pixel (sx*s, sy*s).
 *   model     model_depth [n][Hm][Wm] and model_normals [n][3][Hm][Wm]: the depth and normals planes smx_tsdf_raycast
 *             wrote for the view with the reprojection matrix Qm (host 4x4, in the form that entry accepts) and the pose
 *             model_camera_to_world [n][3][4] f32 (device); Pm (host 4x4) is inv(Qm) and model_world_to_camera [n][3][4]
 *             the inverse pose (the Python layer inverts both in float64 and rounds once, as for smx_tsdf_integrate).
 *   pose      pose_in [n][3][4] f32 (device), camera-to-world: T = (R, t) starts as pose_in.
 *   terms     of a selected accepted pixel at the pose T, with Mw = model_world_to_camera[f], Mc = model_camera_to_world[f]:
 *               p_r = ((R_r0*X + R_r1*Y) + R_r2*Z) + t_r                                   r = 0, 1, 2
 *               c_r = ((Mw[r][0]*p_0 + Mw[r][1]*p_1) + Mw[r][2]*p_2) + Mw[r][3];  skip unless c_2 > 0
 *               u_r = ((Pm[r][0]*c_0 + Pm[r][1]*c_1) + Pm[r][2]*c_2) + Pm[r][3]    r = 0, 1, 3;  skip unless u_3 > 0
 *               fu = floorf(u_0/u_3 + 0.5f), fv = floorf(u_1/u_3 + 0.5f); skip unless 0 <= fu <= Wm-1 and 0 <= fv <= Hm-1
 *               lam = model_depth[f][fv][fu]; skip unless lam is finite and > 0
 *               nrm = model_normals[f][.][fv][fu]; skip if all three are 0
 *               X'' = (Qm00*fu + Qm01*fv) + Qm03, Y'' and Z'' likewise; rx = X''/Z'', ry = Y''/Z''
 *               q_r = Mc[r][3] + ((Mc[r][0]*rx + Mc[r][1]*ry) + Mc[r][2])*lam     (smx_tsdf_raycast's p* of that pixel)
 *               dl_r = q_r - p_r; skip unless (dl_0*dl_0 + dl_1*dl_1) + dl_2*dl_2 <= max_distance*max_distance (NaN fails)
 *               b = (nrm_0*dl_0 + nrm_1*dl_1) + nrm_2*dl_2
 *               a = (p_1*nrm_2 - p_2*nrm_1, p_2*nrm_0 - p_0*nrm_2, p_0*nrm_1 - p_1*nrm_0, nrm_0, nrm_1, nrm_2): the row
 *                   of a small world-frame twist (omega, tau) applied on the left, p' = p + omega x p + tau
 *             Thirty terms, each a float32 product converted to float64: k = 0..20 (w*a_i)*a_j for i <= j in the order
 *             (0,0), (0,1), .., (0,5), (1,1), .., (5,5); k = 21..26 (w*a_i)*b; k = 27 (w*b)*b; k = 28 w; k = 29 1 (the
 *             inlier count).  A pixel that is skipped, not accepted or not selected contributes +0.0 to every term.
 *   sums      float64, in an order fixed by (H, W, s) alone.  The selected grid is cut into tiles of 64 columns x 4 rows,
 *             the tiles at the right and lower edges padded with pixels that contribute +0.0.  (1) In every tile column,
 *             starting from +0.0, the rows' terms are added top to bottom.  (2) The 64 column sums of a tile are reduced by
 *             an adjacent-pairs tree: columns 2i and 2i+1 first, then those sums in adjacent pairs, and so on.  (3) The
 *             tile sums, in row-major tile order and padded with +0.0 to a power of two, are reduced by the same tree.
 *   solve     A (symmetric 6x6 from terms 0..20) x = g (terms 21..26) by LDL^T without pivoting in float64: for
 *             j = 0..5: v_k = L_jk*d_k for k < j; d_j = A_jj - L_j0*v_0 - .. - L_j,j-1*v_j-1 (subtracted one at a time in
 *             that order); for i > j: L_ij = (A_ij - L_i0*v_0 - .. - L_i,j-1*v_j-1)/d_j.  Then y_i = g_i - L_i0*y_0 - ..
 *             - L_i,i-1*y_i-1 for i = 0..5, and for i = 5..0: x_i = y_i/d_i - L_i+1,i*x_i+1 - .. - L_5i*x_5.  The triple is
 *             LOST if the inlier count (term 29) is below min_inliers, if a pivot d_j is not finite or <= min_pivot (an
 *             absolute bound: pivots grow with the sum of the weights), or if a component of x is not finite.
 *   update    omega = (f32)(x_0, x_1, x_2), tau = (f32)(x_3, x_4, x_5).  The rotation is the Cayley map of omega, which is
 *             orthogonal by construction and needs no sin or cos: a = omega*0.5f, aa = (a_0*a_0 + a_1*a_1) + a_2*a_2,
 *             den = 1.0f + aa, k = 1.0f - aa, t_i = 2.0f*a_i,
 *               C = | (k + t_0*a_0)/den    (t_0*a_1 - t_2)/den   (t_0*a_2 + t_1)/den |
 *                   | (t_1*a_0 + t_2)/den  (k + t_1*a_1)/den     (t_1*a_2 - t_0)/den |
 *                   | (t_2*a_0 - t_1)/den  (t_2*a_1 + t_0)/den   (k + t_2*a_2)/den   |
 *             R_rc <- (C_r0*R_0c + C_r1*R_1c) + C_r2*R_2c and t_r <- ((C_r0*t_0 + C_r1*t_1) + C_r2*t_2) + tau_r.
 *   schedule  host int32 [schedule_pairs][2] of (stride, iterations), coarse to fine: at most 8 pairs and 64 iterations in
 *             all.  A triple stops, and its later iterations do nothing, when it is LOST, and after an update with
 *             (omega_0^2 + omega_1^2) + omega_2^2 <= rot_eps*rot_eps and the same sum of tau <= trans_eps*trans_eps.
 * Outputs: pose_out [n][3][4] f32 (may be pose_in itself), the pose after the last update; a LOST triple gets pose_in's
 * bits.  Each of the following may be NULL: info [n][4] int32 = (lost, iterations run, the inlier count of the last one
 * run, its selected accepted pixels); rms [n] f32 = sqrtf((f32)(term 27 / term 28)) of the last iteration run (the
 * division in float64), NaN if none ran or no pixel was an inlier; normal_equations [n][30] f64, the thirty sums of the
 * last iteration run (+0.0 if none ran): terms 0..20 are the information matrix of the pose.
 * One launch, then two per iteration (accumulate the sums of every four tiles; combine them, solve, update) on `stream`
 * (a caller's stream), no atomics, no host synchronisation, no allocation: graph-capturable.  The stop flags live in the
 * workspace and the first launch of every call resets them.  The composition of float32 rotations over a long sequence
 * drifts from orthogonality; that, loop closure and relocalisation are the caller's.
 * workspace: smx_track_camera_workspace_bytes(n, H, W) bytes (0 for sizes the call rejects).
 * SMX_ERR_INVALID_ARG, checked before the device is touched: a NULL disp, Q, model_depth, model_normals, Qm, Pm,
 * model_camera_to_world, model_world_to_camera, pose_in, pose_out or workspace; n < 1, H or W outside 1..32768,
 * n*H*W > 2^30 or ceil(W/64)*ceil(H/4) > 32768; Hm or Wm outside 1..32768 or n*Hm*Wm > 2^30; a non-finite Q, Qm or Pm
 * entry or a Qm outside smx_tsdf_raycast's form; a NaN z bound or z_min > z_max; a non-finite min_confidence or
 * invalid_disparity; schedule_pairs outside 0..8, a NULL schedule with pairs, a stride outside 1..32768, a negative
 * iteration count or more than 64 iterations in all; max_distance not finite and > 0; min_inliers < 1; min_pivot, rot_eps
 * or trans_eps not finite and >= 0; workspace_bytes below the query; an output or the workspace overlapping an input
 * (pose_out == pose_in excepted) or another output; stream == SMX_STREAM_ENGINE. */
size_t smx_track_camera_workspace_bytes(int n, int H, int W);
int smx_track_camera(int device_id, int n, int H, int W, const float *disp, const float *confidence, const float Q[16],
                     float min_confidence, float z_min, float z_max, float invalid_disparity, int Hm, int Wm,
                     const float *model_depth, const float *model_normals, const float Qm[16], const float Pm[16],
                     const float *model_camera_to_world, const float *model_world_to_camera, const float *pose_in,
                     int schedule_pairs, const int32_t *schedule, float max_distance, int min_inliers, float min_pivot,
                     float rot_eps, float trans_eps, float *pose_out, int32_t *info, float *rms,
                     double *normal_equations, void *workspace, size_t workspace_bytes, void *stream);

/* smx_track_camera_photometric: smx_track_camera with a photometric term summed into the same 6 x 6 system, so that
 * texture holds the directions that geometry leaves free (a frame that sees one plane).  Arguments, pixel rule, sums,
 * solve, update, schedule, stop rule and launches are smx_track_camera's; what follows is what is added.  Every step is
 * ONE float32 operation, as there.
 *   planes    frame_intensity [n][H][W] f32 (the frame's pixels) and model_intensity [n][Hm][Wm] f32 (the model view's),
 *             in one unit of the caller's choice (smx_intensity_planes gives 0..255); photometric_weight lambda, in metres
 *             per intensity unit, scales an intensity residual to the geometric residuals' metres.
 *   terms     A selected pixel contributes smx_track_camera's thirty terms by that rule, unchanged.  If, and only if, it
 *             was an inlier there (it reached term 29), with that rule's p, u_0, u_1, u_3, w, Mw and Pm:
 *               x = u_0/u_3, y = u_1/u_3; x0 = floorf(x), y0 = floorf(y); skip unless 0 <= x0 <= Wm-2 and 0 <= y0 <= Hm-2
 *               the taps (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1): skip unless model_depth is finite and > 0 at all
 *                 four and model_intensity is finite at all four: I00, I10, I01, I11
 *               ax = x - x0, ay = y - y0, bx = 1.0f - ax, by = 1.0f - ay
 *               Im = by*(bx*I00 + ax*I10) + ay*(bx*I01 + ax*I11)            (the bilinear interpolant ...
 *               gx = by*(I10 - I00) + ay*(I11 - I01)
 *               gy = bx*(I01 - I00) + ax*(I11 - I10)                          ... and its exact gradient)
 *               e = frame_intensity[f][py][px] - Im; skip unless e is finite and |e| <= max_intensity_difference
 *               h_j = (gx*(Pm[0][j] - x*Pm[3][j]) + gy*(Pm[1][j] - y*Pm[3][j]))/u_3     j = 0, 1, 2 (model camera frame)
 *               gw_i = (Mw[0][i]*h_0 + Mw[1][i]*h_1) + Mw[2][i]*h_2                    i = 0, 1, 2 (world frame)
 *               a' = (lambda*(p_1*gw_2 - p_2*gw_1), lambda*(p_2*gw_0 - p_0*gw_2), lambda*(p_0*gw_1 - p_1*gw_0),
 *                     lambda*gw_0, lambda*gw_1, lambda*gw_2), b' = lambda*e; skip unless all seven are finite
 *             Its terms, float32 products converted to float64: k = 0..20 (w*a'_i)*a'_j and k = 21..26 (w*a'_i)*b' are
 *             added into the SAME sums as the geometric terms k; per pixel and per sum the geometric term is added to the
 *             tile column's sum first and the photometric one second.  Terms 27, 28, 29 and the accepted count stay
 *             geometric, so rms, inliers, min_inliers and the LOST rule mean what they mean in smx_track_camera.  Three
 *             new sums, reduced in the same order: k = 30 (w*e)*e, k = 31 w, k = 32 1 (the photometric inlier count).
 *             With lambda = 0 every photometric product is +-0.0 and changes no bit: pose_out, info, rms and sums 0..29
 *             are smx_track_camera's.
 * Outputs as smx_track_camera's, except that normal_equations is [n][33] f64 (sums 0..29 of the joint system, then the
 * three photometric sums); and, each may be NULL: photometric_info [n][2] int32 = (the photometric inlier count of the
 * last iteration run, its geometric inliers without a photometric term), photometric_rms [n] f32 =
 * sqrtf((f32)(sum 30 / sum 31)) of the last iteration run (the division in float64), in intensity units, NaN if none ran
 * or no pixel was a photometric inlier.  The term's basin is a few model pixels; smx_track_camera_pyramid below reads
 * the term coarse to fine from pyramids and weighs it by Huber's rule.  Neither entry compensates exposure or gain, and
 * the geometric term has no pyramid: it reads the full-resolution depth and normals at every stride.
 * workspace: smx_track_camera_photometric_workspace_bytes(n, H, W) bytes (0 for sizes the call rejects).
 * SMX_ERR_INVALID_ARG: a NULL frame_intensity or model_intensity; everything smx_track_camera rejects; photometric_weight
 * not finite and >= 0; max_intensity_difference not finite and > 0; the overlap rule with the planes among the inputs and
 * photometric_info and photometric_rms among the outputs. */
size_t smx_track_camera_photometric_workspace_bytes(int n, int H, int W);
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
                                 void *workspace, size_t workspace_bytes, void *stream);

/* smx_intensity_planes: image uint8 [n][channels][H][W] (device) to out f32 [n][H][W], the planes the entry above reads.
 * channels == 3 (R, G, B): (float)(77*R + 150*G + 29*B) * 0.00390625f, which is exact; channels == 1: (float)v.  One
 * launch on `stream` (a caller's stream).  SMX_ERR_INVALID_ARG: a NULL image or out; n < 1, H or W outside 1..32768,
 * n*H*W > 2^30; channels other than 1 or 3; out overlapping image; stream == SMX_STREAM_ENGINE. */
int smx_intensity_planes(int device_id, int n, int channels, int H, int W, const uint8_t *image, float *out,
                         void *stream);

/* smx_intensity_pyramid: the Gaussian pyramid of n float32 planes [n][H][W] (device), the operand of
 * smx_track_camera_pyramid.  pyramid (device, smx_intensity_pyramid_bytes(n, H, W, levels) bytes; 0 for arguments the
 * call rejects) holds level 0, then level 1, and so on; level l is [n][H_l][W_l] f32 with H_0 = H, H_(l+1) = (H_l + 1)/2
 * in integers, and W alike: ceil(H / 2^l), the selected grid of stride 2^l.
 *   level 0   plane; where mask_depth ([n][H][W] f32, may be NULL) is given and is not finite and > 0 at a pixel, a NaN.
 *   level l+1 Burt and Adelson's reduce of level l = a [H_l][W_l]: pixel (x, y) sits on a's pixel (2x, 2y).  Every step is
 *             ONE float32 operation; column indices are clamped to 0..W_l-1 and row indices to 0..H_l-1:
 *               h(r, x) = (((a[r][2x-2] + a[r][2x+2]) + 4.0f*(a[r][2x-1] + a[r][2x+1])) + 6.0f*a[r][2x]) * 0.0625f
 *               out(x, y) = (((h(2y-2, x) + h(2y+2, x)) + 4.0f*(h(2y-1, x) + h(2y+1, x))) + 6.0f*h(2y, x)) * 0.0625f
 *             NaNs and infinities propagate by that arithmetic: a level pixel with a NaN in its 5 x 5 footprint is a NaN,
 *             which is how model pixels without a surface stay out of the photometric term at every level.
 * One launch per level on `stream` (a caller's stream); no workspace, no atomics.
 * SMX_ERR_INVALID_ARG: a NULL plane or pyramid; n < 1, H or W outside 1..32768, n*H*W > 2^30; levels outside 1..8; pyramid
 * overlapping plane or mask_depth; stream == SMX_STREAM_ENGINE. */
size_t smx_intensity_pyramid_bytes(int n, int H, int W, int levels);
int smx_intensity_pyramid(int device_id, int n, int H, int W, int levels, const float *plane, const float *mask_depth,
                          float *pyramid, void *stream);

/* smx_track_camera_pyramid: smx_track_camera_photometric with the photometric term read from a level of two intensity
 * pyramids per schedule pair, coarse to fine, and weighed by Huber's rule, so that the term pulls from starts many
 * pixels off.  Arguments, geometric terms (from the full-resolution depth and normals at every stride), sums, solve,
 * update, LOST rule, stop rule, outputs, workspace (smx_track_camera_photometric_workspace_bytes) and launches are that
 * entry's; what follows is what differs.
 *   pyramids  frame_pyramid of (n, H, W) and model_pyramid of (n, Hm, Wm), both of `levels` levels in
 *             smx_intensity_pyramid's layout, in place of the two planes.  The model's is built with mask_depth =
 *             model_depth, so the term has no depth test of its own.  schedule_levels (host) [schedule_pairs] int32: the
 *             level l of every pair, with 2^l dividing the pair's stride s, so that a selected pixel (px, py) is the
 *             level's pixel (px >> l, py >> l) exactly.  huber_delta, in intensity units; +inf: no robust weights.
 *   terms     Of a geometric inlier in a pair of level l, with inv = 2^-l, Wl, Hl the model pyramid's dimensions at level
 *             l and x, y, u_3 of smx_track_camera_photometric:
 *               xl = x*inv, yl = y*inv; x0 = floorf(xl), y0 = floorf(yl); skip unless 0 <= x0 <= Wl-2 and 0 <= y0 <= Hl-2
 *               the four taps from the model's level l: skip unless all four are finite
 *               ax = xl - x0, ay = yl - y0; bx, by, Im as there, and the level's gradient gxl, gyl as gx, gy there
 *               gx = gxl*inv, gy = gyl*inv                                          (per level-0 pixel; exact)
 *               e = frame_pyramid[l][f][py >> l][px >> l] - Im; skip unless e is finite and |e| <= max_intensity_difference
 *               h, gw, a', b' and the finiteness test as there, with the level-0 x, y and u_3
 *               wh = |e| <= huber_delta ? 1.0f : huber_delta/|e|; wp = w*wh
 *             wp takes w's place in the photometric products: k = 0..20 (wp*a'_i)*a'_j, k = 21..26 (wp*a'_i)*b',
 *             k = 30 (wp*e)*e, k = 31 wp, k = 32 1.  With every level 0 and huber_delta = +inf every added operation is a
 *             multiplication by 1.0f: on pyramids whose level 0 is the frame's plane and the model's plane masked by
 *             model_depth, the entry returns smx_track_camera_photometric's bits.
 * SMX_ERR_INVALID_ARG: everything smx_track_camera_photometric rejects (a NULL frame_pyramid or model_pyramid; the overlap
 * rule over the whole pyramids); levels outside 1..8; a NULL schedule_levels with schedule_pairs > 0; a level outside
 * 0..levels-1; a stride not divisible by 2^level; huber_delta NaN or <= 0.  Not here: exposure or gain compensation,
 * robust weights or a pyramid for the geometric term. */
int smx_track_camera_pyramid(int device_id, int n, int H, int W, const float *disp, const float *confidence,
                             const float Q[16], float min_confidence, float z_min, float z_max, float invalid_disparity,
                             int Hm, int Wm, const float *model_depth, const float *model_normals, const float Qm[16],
                             const float Pm[16], const float *model_camera_to_world, const float *model_world_to_camera,
                             const float *pose_in, int schedule_pairs, const int32_t *schedule, float max_distance,
                             int min_inliers, float min_pivot, float rot_eps, float trans_eps, const float *frame_pyramid,
                             const float *model_pyramid, int levels, const int32_t *schedule_levels,
                             float photometric_weight, float max_intensity_difference, float huber_delta, float *pose_out,
                             int32_t *info, float *rms, double *normal_equations, int32_t *photometric_info,
                             float *photometric_rms, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
