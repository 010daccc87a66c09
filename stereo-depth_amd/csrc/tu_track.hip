// tu_track.hip -- camera tracking against a rendered model view (k_track.h): one launch that takes the poses in, then
// two launches per iteration of the schedule (k_track_body.h: track_launch).
#include "k_track.h"

namespace smx {

void launch_track_camera(const TrackCall &c, hipStream_t s) {
    TrackArgs a;
    track_launch<TrackRule>(c, a, k_track_begin, k_track_accum, k_track_solve, s);
}

}  // namespace smx
