// k_track_pyramid.h -- camera tracking with the photometric term read coarse to fine from intensity pyramids and weighed
// by Huber's rule (smx_track_camera_pyramid): k_track_body.h's launches for the joint rule over k_track_pyramid_rule.h's
// record.  The rule, bit for bit, is in include/stereo_mi355x.h; tests/track_pyramid_ref.py restates it in NumPy.
//
// The sums are the joint rule's, so the slots are its slots and the combine has k_track_photo.h's shape: that header
// holds kernels, so this unit cannot include it, and states the two numbers again (tests/test_track_pyramid_abi.py
// compares them).
#pragma once
#include "k_track_body.h"
#include "k_track_pyramid_rule.h"

namespace smx {

constexpr int TRKY_CHUNKS = 16;                                       // TRKP_CHUNKS
constexpr int TRKY_STACK = 7;                                         // TRKP_STACK

using TrackPyramidRule = TrackJointRule<TrackPyramidArgs, TRKY_CHUNKS, TRKY_STACK>;

__global__ __launch_bounds__(256) void k_track_pyramid_begin(const TrackPyramidArgs a) { track_begin_body<TrackPyramidRule>(a); }
__global__ __launch_bounds__(256) void k_track_pyramid_accum(const TrackPyramidArgs a) { track_accum_body<TrackPyramidRule>(a); }
__global__ __launch_bounds__(1024) void k_track_pyramid_solve(const TrackPyramidArgs a) { track_solve_body<TrackPyramidRule>(a); }

}  // namespace smx
