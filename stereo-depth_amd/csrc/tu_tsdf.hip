// tu_tsdf.hip -- TSDF fusion of posed disparity maps and the extraction of the volume's surface as points (k_tsdf.h)
// and as triangles over those points (k_mesh.h).
#include <cstring>

#include "k_mesh.h"
#include "k_tsdf.h"
#include "smx_launch.h"
#include "smx_workspace.h"

namespace smx {

void launch_tsdf_integrate(int nx, int ny, int nz, const float origin[3], float voxel_size, float truncation,
                           float max_weight, float *tsdf, float *weight, uint8_t *color, int n, int H, int W,
                           const float *disp, const float q[16], const float p[16], const float *world_to_camera,
                           const float *conf, float min_conf, float zmin, float zmax, float invalid, const void *image,
                           int channels, bool img_f32, void *workspace, hipStream_t s) {
    TsdfArgs a;
    a.nx = nx, a.ny = ny, a.nz = nz;
    a.ox = origin[0], a.oy = origin[1], a.oz = origin[2], a.s = voxel_size, a.tau = truncation;
    a.max_weight = max_weight;
    a.tsdf = tsdf, a.weight = weight, a.color = (unsigned *)color;
    a.n = n, a.H = H, a.W = W;
    a.disp = disp, a.conf = conf;
    std::memcpy(a.q, q, sizeof(a.q));
    std::memcpy(a.p, p, sizeof(a.p));
    a.pose = world_to_camera;
    a.min_conf = min_conf, a.zmin = zmin, a.zmax = zmax, a.invalid = invalid;
    a.image = image, a.channels = image ? channels : 0, a.img_f32 = img_f32 ? 1 : 0;
    const size_t px = (size_t)n * H * W;
    const TsdfIntegrateLayout l = tsdf_integrate_layout(n, H, W);
    a.meas = ws_at<float2>(workspace, l.meas), a.pcol = ws_at<unsigned>(workspace, l.pcol);
    hipLaunchKernelGGL(k_tsdf_pixels, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)((nx + 63) / 64), (unsigned)((ny + 3) / 4), (unsigned)nz),
                       dim3(256), 0, s, a);
}

void launch_tsdf_extract(int nx, int ny, int nz, const float origin[3], float voxel_size, const float *tsdf,
                         const float *weight, const uint8_t *color, float min_weight, int capacity, float *points,
                         float *normals, uint8_t *colors, int32_t *count, void *workspace, hipStream_t s) {
    TsdfExtractArgs a;
    a.nx = nx, a.ny = ny, a.nz = nz;
    a.ox = origin[0], a.oy = origin[1], a.oz = origin[2], a.s = voxel_size, a.min_weight = min_weight;
    a.tsdf = tsdf, a.weight = weight, a.color = (const unsigned *)color;
    a.capacity = (unsigned)capacity;
    a.points = points, a.normals = normals, a.colors = color ? colors : nullptr, a.count = count;
    const long rows = (long)ny * nz;
    const TsdfExtractLayout l = tsdf_extract_layout(ny, nz);
    a.row_count = ws_at<int>(workspace, l.row_count), a.row_offset = ws_at<int>(workspace, l.row_offset);
    int *block_sums = ws_at<int>(workspace, l.block_sums);
    hipLaunchKernelGGL(k_tsdf_count, dim3((unsigned)rows), dim3(256), 0, s, a);
    launch_scan(a.row_count, a.row_offset, rows, block_sums, nullptr, 0, s);
    hipLaunchKernelGGL(k_tsdf_scatter, dim3((unsigned)rows), dim3(256), 0, s, a);
}

void launch_tsdf_triangles(int nx, int ny, int nz, const float *tsdf, const float *weight, float min_weight,
                           int capacity, int32_t *triangles, int32_t *count, void *workspace, hipStream_t s) {
    const MeshLayout l = mesh_layout(nx, ny, nz);
    MeshArgs a;
    a.v = TsdfExtractArgs{};
    a.v.nx = nx, a.v.ny = ny, a.v.nz = nz, a.v.min_weight = min_weight;
    a.v.tsdf = tsdf, a.v.weight = weight;
    const long rows = (long)ny * nz;
    int *counts = ws_at<int>(workspace, l.counts), *offsets = ws_at<int>(workspace, l.offsets);
    a.v.row_count = counts, a.v.row_offset = offsets;
    a.tri_hi = counts + rows, a.tri_hi_offset = offsets + rows;
    a.tri_count = counts + 2 * rows, a.tri_offset = offsets + 2 * rows;
    a.nch = l.nch;
    a.flags = ws_at<uint8_t>(workspace, l.flags), a.chunk_first = ws_at<unsigned>(workspace, l.chunk_first);
    a.capacity = (unsigned)capacity, a.triangles = triangles, a.count = count;
    int *block_sums = ws_at<int>(workspace, l.block_sums);
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipLaunchKernelGGL(k_mesh_flags, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_mesh_count, grid, dim3(256), 0, s, a);
    launch_scan(counts, offsets, 3 * rows, block_sums, nullptr, 0, s);
    hipLaunchKernelGGL(k_mesh_scatter, grid, dim3(256), 0, s, a);
}

}  // namespace smx
