// tu_track_photo.hip -- camera tracking with the photometric term (k_track_photo.h): one launch that takes the poses in,
// then two launches per iteration of the schedule (k_track_body.h: track_launch); and the intensity planes of uint8
// frames, one launch.
#include "k_track_photo.h"

namespace smx {

void launch_track_camera_photometric(const TrackCall &c, const TrackPhotoTerm &t, hipStream_t s) {
    TrackPhotoArgs a;
    a.frame_int = t.frame_intensity, a.model_int = t.model_intensity;
    a.weight = t.weight, a.max_diff = t.max_intensity_difference;
    a.pinfo = t.info, a.prms = t.rms;
    track_launch<TrackPhotoRule>(c, a, k_track_photo_begin, k_track_photo_accum, k_track_photo_solve, s);
}

void launch_intensity_planes(int n, int C, int H, int W, const uint8_t *in, float *out, hipStream_t s) {
    const size_t plane = (size_t)H * W, total = (size_t)n * plane;
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_intensity_planes, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, in, out, C,
                       plane, total);
}

}  // namespace smx
