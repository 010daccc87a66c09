// k_track.h -- frame-to-model camera tracking by projective point-to-plane ICP (smx_track_camera): k_track_body.h's
// launches for the geometric rule.  The rule, bit for bit, is in include/stereo_mi355x.h; k_track_rule.h holds its
// per-pixel terms and its solve as host/device code, and tests/track_ref.py restates it in NumPy.
#pragma once
#include "k_track_body.h"

namespace smx {

constexpr int TRK_CHUNKS = 32;                                        // chunks of consecutive partials per triple: 32 lanes each
constexpr int TRK_STACK = 6;                                          // levels above a leaf of 8: chunks of up to 256 partials

struct TrackRule {
    using Args = TrackArgs;
    static constexpr int SLOTS = TRK_SLOTS, BUTTERFLY = TRK_TERMS + 1, CHUNKS = TRK_CHUNKS, STACK = TRK_STACK;
    static SMX_FN TrackArgs &common(TrackArgs &a) { return a; }
    static SMX_FN const TrackArgs &common(const TrackArgs &a) { return a; }
    static SMX_FN void pixel(const TrackArgs &a, const float *T, int f, int px, int py, double *acc) {
        trk_pixel(a, T, f, px, py, acc);
    }
    static SMX_FN void begin(const TrackArgs &a, int f) { trk_begin(a, f); }
    static SMX_FN void finish(const TrackArgs &a, int f, const double *S) { trk_finish(a, f, S); }
};

__global__ __launch_bounds__(256) void k_track_begin(const TrackArgs a) { track_begin_body<TrackRule>(a); }
__global__ __launch_bounds__(256) void k_track_accum(const TrackArgs a) { track_accum_body<TrackRule>(a); }
__global__ __launch_bounds__(1024) void k_track_solve(const TrackArgs a) { track_solve_body<TrackRule>(a); }

}  // namespace smx
