// k_track_photo.h -- camera tracking with a photometric term summed into the geometric system
// (smx_track_camera_photometric): k_track_body.h's launches for the joint rule, and the intensity planes it reads
// (smx_intensity_planes).  The rule, bit for bit, is in include/stereo_mi355x.h; k_track_photo_rule.h holds its per-pixel
// terms as host/device code, and tests/track_photo_ref.py restates it in NumPy.
//
// 34 slots do not fit 32 lanes, so a wave is a chunk of the combine here: 16 chunks, the lanes past TRKP_SLOTS idle, and
// a wave reads TRKP_SLOTS consecutive doubles of a partial at a time.
#pragma once
#include "k_track_body.h"
#include "k_track_photo_rule.h"

namespace smx {

constexpr int TRKP_CHUNKS = 16;                                       // chunks of consecutive partials per triple: one wave each
constexpr int TRKP_STACK = 7;                                         // levels above a leaf of 8: chunks of up to 512 partials

using TrackPhotoRule = TrackJointRule<TrackPhotoArgs, TRKP_CHUNKS, TRKP_STACK>;

__global__ __launch_bounds__(256) void k_track_photo_begin(const TrackPhotoArgs a) { track_begin_body<TrackPhotoRule>(a); }
__global__ __launch_bounds__(256) void k_track_photo_accum(const TrackPhotoArgs a) { track_accum_body<TrackPhotoRule>(a); }
__global__ __launch_bounds__(1024) void k_track_photo_solve(const TrackPhotoArgs a) { track_solve_body<TrackPhotoRule>(a); }

// uint8 [n][C][H][W] -> f32 [n][H][W]: grid-stride over the pixels, one thread per pixel
__global__ __launch_bounds__(256) void k_intensity_planes(const uint8_t *__restrict__ in, float *__restrict__ out, int C,
                                                          size_t plane, size_t total) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        if (C == 1) {
            out[i] = (float)in[i];
        } else {
            const size_t f = i / plane;
            const uint8_t *p = in + 2 * f * plane + i;                // frame f's R plane starts at 3 f plane
            const int r = p[0], g = p[plane], b = p[2 * plane];
            out[i] = (float)(77 * r + 150 * g + 29 * b) * 0.00390625f;
        }
    }
}

}  // namespace smx
