// tu_tsdf.hip -- TSDF fusion of posed disparity maps and the extraction of the volume's surface as points (k_tsdf.h)
// and as triangles over those points (k_mesh.h).
#include <cstring>

#include "k_mesh.h"
#include "k_tsdf.h"
#include "smx_launch.h"

namespace smx {

static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// [n*H*W] float2 measurements, then [n*H*W] colour words
size_t tsdf_integrate_workspace_bytes(int n, int H, int W) {
    const size_t px = (size_t)n * H * W;
    return align256(px * sizeof(float2)) + align256(px * sizeof(unsigned));
}

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
    a.meas = (float2 *)workspace;
    a.pcol = (unsigned *)((char *)workspace + align256(px * sizeof(float2)));
    hipLaunchKernelGGL(k_tsdf_pixels, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)((nx + 63) / 64), (unsigned)((ny + 3) / 4), (unsigned)nz),
                       dim3(256), 0, s, a);
}

// [rows] counts, [rows] offsets, the scan's block sums
size_t tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
    (void)nx;
    const long rows = (long)ny * nz;
    return 2 * align256((size_t)rows * sizeof(int)) + align256(scan_block_sums(rows) * sizeof(int));
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
    char *ws = (char *)workspace;
    a.row_count = (int *)ws;
    a.row_offset = (int *)(ws + align256((size_t)rows * sizeof(int)));
    int *block_sums = (int *)(ws + 2 * align256((size_t)rows * sizeof(int)));
    hipLaunchKernelGGL(k_tsdf_count, dim3((unsigned)rows), dim3(256), 0, s, a);
    launch_scan(a.row_count, a.row_offset, rows, block_sums, nullptr, 0, s);
    hipLaunchKernelGGL(k_tsdf_scatter, dim3((unsigned)rows), dim3(256), 0, s, a);
}

namespace {
struct MeshLayout {
    size_t flags, chunk_first, counts, offsets, block_sums, total;
    int nch;
};

// one byte per voxel, one word per 64-voxel chunk of a row, three counts and three offsets per row, the scan's block sums
MeshLayout mesh_layout(int nx, int ny, int nz) {
    MeshLayout l;
    const size_t rows = (size_t)ny * nz;
    l.nch = (nx + 63) / 64;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    l.flags = take(rows * nx);
    l.chunk_first = take(rows * l.nch * sizeof(unsigned));
    l.counts = take(3 * rows * sizeof(int));
    l.offsets = take(3 * rows * sizeof(int));
    l.block_sums = take(scan_block_sums(3 * (long)rows) * sizeof(int));
    l.total = at;
    return l;
}
}  // namespace

size_t tsdf_triangles_workspace_bytes(int nx, int ny, int nz) { return mesh_layout(nx, ny, nz).total; }

void launch_tsdf_triangles(int nx, int ny, int nz, const float *tsdf, const float *weight, float min_weight,
                           int capacity, int32_t *triangles, int32_t *count, void *workspace, hipStream_t s) {
    const MeshLayout l = mesh_layout(nx, ny, nz);
    char *ws = (char *)workspace;
    MeshArgs a;
    a.v = TsdfExtractArgs{};
    a.v.nx = nx, a.v.ny = ny, a.v.nz = nz, a.v.min_weight = min_weight;
    a.v.tsdf = tsdf, a.v.weight = weight;
    const long rows = (long)ny * nz;
    int *counts = (int *)(ws + l.counts), *offsets = (int *)(ws + l.offsets);
    a.v.row_count = counts, a.v.row_offset = offsets;
    a.tri_hi = counts + rows, a.tri_hi_offset = offsets + rows;
    a.tri_count = counts + 2 * rows, a.tri_offset = offsets + 2 * rows;
    a.nch = l.nch;
    a.flags = (uint8_t *)(ws + l.flags), a.chunk_first = (unsigned *)(ws + l.chunk_first);
    a.capacity = (unsigned)capacity, a.triangles = triangles, a.count = count;
    int *block_sums = (int *)(ws + l.block_sums);
    const dim3 grid((unsigned)((rows + 3) / 4));
    hipLaunchKernelGGL(k_mesh_flags, grid, dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_mesh_count, grid, dim3(256), 0, s, a);
    launch_scan(counts, offsets, 3 * rows, block_sums, nullptr, 0, s);
    hipLaunchKernelGGL(k_mesh_scatter, grid, dim3(256), 0, s, a);
}

}  // namespace smx
