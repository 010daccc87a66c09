// tu_track_photo.hip -- camera tracking with the photometric term (k_track_photo.h): one launch that takes the poses in,
// then two launches per iteration of the schedule; and the intensity planes of uint8 frames, one launch.
#include <cstring>

#include "k_track_photo.h"
#include "smx_launch.h"
#include "smx_workspace.h"

namespace smx {

void launch_track_camera_photometric(int n, int H, int W, const float *disp, const float *confidence, const float q[16],
                                     float min_confidence, float zmin, float zmax, float invalid, int Hm, int Wm,
                                     const float *model_depth, const float *model_normals, const float qm[16],
                                     const float pm[16], const float *model_camera_to_world,
                                     const float *model_world_to_camera, const float *pose_in, int pairs,
                                     const int32_t *schedule, float max_distance, int min_inliers, float min_pivot,
                                     float rot_eps, float trans_eps, const float *frame_intensity,
                                     const float *model_intensity, float photometric_weight,
                                     float max_intensity_difference, float *pose_out, int32_t *info, float *rms,
                                     double *normal_equations, int32_t *photometric_info, float *photometric_rms,
                                     void *workspace, hipStream_t s) {
    const TrackLayout l = track_photo_layout(n, H, W);
    TrackPhotoArgs pa;
    TrackArgs &a = pa.g;
    a.n = n, a.H = H, a.W = W, a.Hm = Hm, a.Wm = Wm;
    a.disp = disp, a.conf = confidence, a.depth = model_depth, a.normals = model_normals;
    a.c2w = model_camera_to_world, a.w2c = model_world_to_camera;
    std::memcpy(a.q, q, sizeof(a.q));
    std::memcpy(a.qm, qm, sizeof(a.qm));
    std::memcpy(a.pm, pm, sizeof(a.pm));
    a.min_conf = min_confidence, a.zmin = zmin, a.zmax = zmax, a.invalid = invalid;
    a.maxd2 = max_distance * max_distance;
    a.stride = 1, a.ws = a.hs = a.tx = a.tiles = a.groups = 0;
    a.min_inliers = min_inliers, a.min_pivot = (double)min_pivot;
    a.rot_eps2 = rot_eps * rot_eps, a.trans_eps2 = trans_eps * trans_eps;
    a.pose_in = pose_in, a.pose_out = pose_out, a.rms = rms, a.info = info;
    a.sums = nullptr, a.partial = nullptr, a.partial_stride = 0;     // the joint sums are TrackPhotoArgs's
    a.state = ws_at<TrackState>(workspace, l.state);
    pa.frame_int = frame_intensity, pa.model_int = model_intensity;
    pa.weight = photometric_weight, pa.max_diff = max_intensity_difference;
    pa.pinfo = photometric_info, pa.prms = photometric_rms, pa.sums = normal_equations;
    pa.partial = ws_at<double>(workspace, l.partial);
    pa.partial_stride = (size_t)l.groups * TRKP_SLOTS;
    const unsigned triples = (unsigned)(n < 65535 ? n : 65535);
    hipLaunchKernelGGL(k_track_photo_begin, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pa);
    for (int p = 0; p < pairs; ++p) {
        const TrackGrid g = track_grid(H, W, schedule[2 * p]);
        a.stride = schedule[2 * p], a.ws = g.ws, a.hs = g.hs, a.tx = g.tx, a.tiles = g.tiles, a.groups = g.groups;
        for (int it = 0; it < schedule[2 * p + 1]; ++it) {
            hipLaunchKernelGGL(k_track_photo_accum, dim3((unsigned)g.groups, triples), dim3(256), 0, s, pa);
            hipLaunchKernelGGL(k_track_photo_solve, dim3(triples), dim3(1024), 0, s, pa);
        }
    }
}

void launch_intensity_planes(int n, int C, int H, int W, const uint8_t *in, float *out, hipStream_t s) {
    const size_t plane = (size_t)H * W, total = (size_t)n * plane;
    const size_t blocks = (total + 255) / 256;
    hipLaunchKernelGGL(k_intensity_planes, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, in, out, C,
                       plane, total);
}

}  // namespace smx
