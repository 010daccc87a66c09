// tu_raycast.hip -- views of a TSDF volume by ray casting (k_raycast.h): the two brick passes, then the march.
#include <cstring>

#include "k_raycast.h"
#include "smx_launch.h"
#include "smx_workspace.h"

namespace smx {

void launch_tsdf_raycast(int nx, int ny, int nz, const float origin[3], float voxel_size, const float *tsdf,
                         const float *weight, const uint8_t *color, float min_weight, int n, int H, int W,
                         const float q[16], const float *camera_to_world, float step, float zmin, int M, float invalid,
                         float *disp, float *depth, float *normals, uint8_t *colors, float *out_weight, void *workspace,
                         hipStream_t s) {
    const RaycastLayout l = raycast_layout(nx, ny, nz);
    RaycastArgs a;
    a.nx = nx, a.ny = ny, a.nz = nz;
    a.bx = l.bx, a.by = l.by, a.bz = l.bz;
    a.ox = origin[0], a.oy = origin[1], a.oz = origin[2], a.s = voxel_size, a.min_weight = min_weight;
    a.tsdf = tsdf, a.weight = weight, a.color = (const unsigned *)color;
    a.n = n, a.H = H, a.W = W, a.M = M;
    std::memcpy(a.q, q, sizeof(a.q));
    a.pose = camera_to_world;
    a.step = step, a.zmin = zmin, a.invalid = invalid;
    a.disp = disp, a.depth = depth, a.normals = normals, a.out_weight = out_weight;
    a.colors = color ? colors : nullptr;
    a.flags = ws_at<uint8_t>(workspace, l.flags), a.occ = ws_at<uint8_t>(workspace, l.occ);
    hipLaunchKernelGGL(k_raycast_bricks, dim3((unsigned)l.by, (unsigned)l.bz), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_raycast_free, dim3((unsigned)((l.bx * l.by * l.bz + 255) / 256)), dim3(256), 0, s, a);
    constexpr int TILE_W = RC_TW * RC_BW, TILE_H = RC_TH * RC_BH;
    hipLaunchKernelGGL(k_raycast_march, dim3((unsigned)((W + TILE_W - 1) / TILE_W), (unsigned)((H + TILE_H - 1) / TILE_H),
                                             (unsigned)(n < 65535 ? n : 65535)), dim3(256), 0, s, a);
}

}  // namespace smx
