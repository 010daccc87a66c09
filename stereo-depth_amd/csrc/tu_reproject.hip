// tu_reproject.hip -- reprojection of disparity maps to metric 3D points and voxel-grid downsampling (k_reproject.h).
#include <algorithm>
#include <cstring>

#include "k_reproject.h"
#include "smx_launch.h"
#include "smx_workspace.h"

namespace smx {

void launch_reproject(int n, int H, int W, const float *disp, const float q[16], const float *conf, float min_conf,
                      float zmin, float zmax, float invalid, const void *image, int channels, bool img_f32,
                      float *points, uint8_t *colors, int32_t *indices, float *xyz_map, int32_t *offsets,
                      void *workspace, hipStream_t s) {
    ReprojArgs a;
    a.disp = disp, a.conf = conf, a.image = image, a.channels = image ? channels : 0, a.img_f32 = img_f32 ? 1 : 0;
    std::memcpy(a.q, q, sizeof(a.q));
    a.min_conf = min_conf, a.zmin = zmin, a.zmax = zmax, a.invalid = invalid;
    a.points = points, a.colors = image ? colors : nullptr, a.indices = indices, a.xyz_map = xyz_map;
    a.offsets = offsets;
    a.row_count = ws_at<int>(workspace, reproject_layout(n, H).rows);
    a.row_offset = a.row_count + (size_t)n * H;
    a.n = n, a.H = H, a.W = W;
    const unsigned rows = (unsigned)(n * H);
    hipLaunchKernelGGL(k_reproj_count, dim3(rows), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_reproj_scan, dim3(1), dim3(1024), 0, s, a);
    hipLaunchKernelGGL(k_reproj_scatter, dim3(rows), dim3(256), 0, s, a);
}

void launch_scan(const int *in, int *out, long L, int *block_sums, const int *gate, int pass, hipStream_t s) {
    const int nb = (int)scan_block_sums(L);
    hipLaunchKernelGGL(k_scan_reduce, dim3(nb), dim3(256), 0, s, in, L, block_sums, gate, pass);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, s, block_sums, nb, gate, pass);
    hipLaunchKernelGGL(k_scan_down, dim3(nb), dim3(256), 0, s, in, out, L, block_sums, gate, pass);
}

hipError_t launch_voxel_downsample(int n, int cap, const float *points, const uint8_t *colors, const int32_t *offsets,
                                   float voxel_size, int min_points, float *out_points, uint8_t *out_colors,
                                   int32_t *out_counts, int32_t *out_offsets, int32_t *dropped, void *workspace,
                                   hipStream_t s) {
    const VoxLayout l = vox_layout(n, cap);
    VoxArgs a;
    a.points = points, a.colors = colors, a.offsets_in = offsets, a.voxel_size = voxel_size;
    a.min_points = min_points, a.n = n, a.cap = cap;
    a.out_points = out_points, a.out_colors = colors ? out_colors : nullptr, a.out_counts = out_counts;
    a.out_offsets = out_offsets, a.dropped = dropped;
    a.keys[0] = ws_at<unsigned long long>(workspace, l.keys), a.keys[1] = a.keys[0] + cap;
    a.vals[0] = ws_at<int>(workspace, l.vals), a.vals[1] = a.vals[0] + cap;
    a.counts = ws_at<int>(workspace, l.counts), a.counts_scan = ws_at<int>(workspace, l.counts_scan);
    a.flag = ws_at<int>(workspace, l.flag), a.pos = ws_at<int>(workspace, l.pos), a.vcnt = ws_at<int>(workspace, l.vcnt);
    a.block_sums = ws_at<int>(workspace, l.block_sums);
    a.off = ws_at<int>(workspace, l.off), a.tile_base = ws_at<int>(workspace, l.tile_base);
    a.meta = ws_at<int>(workspace, l.meta);
    // the tail of the histogram array past this call's tiles is scanned too: keep it zero
    hipError_t e = hipMemsetAsync(a.counts, 0, (size_t)l.Lc * sizeof(int), s);
    if (e != hipSuccess) return e;
    const unsigned pts_blocks = (unsigned)((cap + 255) / 256);
    const unsigned tiles = (unsigned)l.max_tiles;
    hipLaunchKernelGGL(k_vox_prep, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_vox_bbox, dim3(std::min<unsigned>(pts_blocks, VOX_BBOX_BLOCKS)), dim3(256), 0, s, a);
    hipLaunchKernelGGL(k_vox_keys, dim3(pts_blocks), dim3(256), 0, s, a);
    const int *gate = a.meta + VM_KEY_BITS;
    for (int pass = 0; pass < 8; ++pass) {                        // the key has at most 64 bits
        hipLaunchKernelGGL(k_vox_hist, dim3(tiles), dim3(256), 0, s, a, pass);
        launch_scan(a.counts, a.counts_scan, l.Lc, a.block_sums, gate, pass, s);
        hipLaunchKernelGGL(k_vox_scatter, dim3(tiles), dim3(256), 0, s, a, pass);
    }
    hipLaunchKernelGGL(k_vox_heads, dim3((unsigned)((l.Lf + 255) / 256)), dim3(256), 0, s, a);
    launch_scan(a.flag, a.pos, l.Lf, a.block_sums, nullptr, 0, s);
    const long reduce_threads = std::max<long>(cap, (long)n + 1);
    hipLaunchKernelGGL(k_vox_reduce, dim3((unsigned)((reduce_threads + 255) / 256)), dim3(256), 0, s, a);
    return hipSuccess;
}

}  // namespace smx
