// tu_track_pyramid.hip -- camera tracking with the photometric term read from intensity pyramids (k_track_pyramid.h): one
// launch that takes the poses in, then two launches per iteration of the schedule (k_track_body.h: track_launch), each
// pair of the schedule with the record of its level.
#include "k_track_pyramid.h"

namespace smx {

void launch_track_camera_pyramid(const TrackCall &c, const TrackPhotoTerm &t, const TrackPyramidTerm &py, hipStream_t s) {
    TrackPyramidArgs a;
    a.frame_lvl = t.frame_intensity, a.model_lvl = t.model_intensity;
    a.shift = 0, a.Hl = c.H, a.Wl = c.W, a.Hml = c.Hm, a.Wml = c.Wm, a.inv = 1.0f;
    a.weight = t.weight, a.max_diff = t.max_intensity_difference, a.huber = py.huber_delta;
    a.pinfo = t.info, a.prms = t.rms;
    track_launch<TrackPyramidRule>(c, a, k_track_pyramid_begin, k_track_pyramid_accum, k_track_pyramid_solve, s,
                                   [&](TrackPyramidArgs &ra, int p) {
                                       const int level = py.schedule_levels[p];
                                       const PyramidLevel fl = pyramid_level(c.n, c.H, c.W, level);
                                       const PyramidLevel ml = pyramid_level(c.n, c.Hm, c.Wm, level);
                                       ra.frame_lvl = t.frame_intensity + fl.offset, ra.model_lvl = t.model_intensity + ml.offset;
                                       ra.shift = level, ra.Hl = fl.H, ra.Wl = fl.W, ra.Hml = ml.H, ra.Wml = ml.W;
                                       ra.inv = 1.0f / (float)(1 << level);
                                   });
}

}  // namespace smx
