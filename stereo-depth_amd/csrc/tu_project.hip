// tu_project.hip -- projection of point clouds into camera views as z-buffered disparity maps (k_project.h).
#include <cstring>

#include "k_project.h"
#include "smx_launch.h"
#include "smx_workspace.h"

namespace smx {

void launch_project(int n, int capacity, int H, int W, const float *points, const int32_t *offsets,
                    const float *world_to_camera, const float p[16], int radius, float zmin, float zmax, float invalid,
                    float *disp, int32_t *index, float *depth, void *workspace, hipStream_t s) {
    const ProjectLayout l = project_layout(n, H, W);
    ProjectArgs a;
    a.points = points, a.offsets_in = offsets, a.w2c = world_to_camera;
    std::memcpy(a.p, p, sizeof(a.p));
    a.zmin = zmin, a.zmax = zmax, a.invalid = invalid;
    a.radius = radius, a.n = n, a.cap = capacity, a.H = H, a.W = W;
    a.disp = disp, a.index = index, a.depth = depth;
    a.keys = ws_at<unsigned long long>(workspace, l.keys), a.off = ws_at<int>(workspace, l.off);
    const unsigned px_blocks = (unsigned)(((size_t)n * H * W + 255) / 256);
    hipLaunchKernelGGL(k_project_clear, dim3(px_blocks), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_project_splat, dim3((unsigned)((capacity + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_project_resolve, dim3(px_blocks), dim3(256), 0, s, a);
}

}  // namespace smx
