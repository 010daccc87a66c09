// raycast_march_harness.cpp -- smx_tsdf_raycast's march on the CPU: the library's own per-pixel rule
// (stereo-depth_amd/csrc/k_raycast_rule.h, the code the kernel runs per thread, jumps included) over every pixel of every
// view, with the brick bytes (empty, measured, free space) computed here from their definition.  tests/test_raycast_march_cpu.py compares its five
// outputs bit for bit with the dense NumPy twin: what the jumps skip must not change a bit.
//
//   raycast_march_harness IN OUT
// IN:  int32 nx ny nz n H W M has_color | f32 ox oy oz s min_weight step zmin invalid | f32 Q[16] | f32 pose[n][12]
//      | f32 tsdf[V] | f32 weight[V] | u32 color[V] (with has_color)
// OUT: f32 disp[P] | f32 depth[P] | f32 normals[3P] | f32 weight[P] | u8 colors[3P] (with has_color), P = n H W
// Prints "raycast-march pixels P bricks B set S free F": the bricks with a measured voxel, and the free ones.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "k_raycast_rule.h"
#include "smx_workspace.h"

template <class T> static void get(FILE *f, T *p, size_t count) {
    if (fread(p, sizeof(T), count, f) != count) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int hd[8];
    float pr[8];
    get(f, hd, 8);
    get(f, pr, 8);
    smx::RaycastArgs a;
    a.nx = hd[0], a.ny = hd[1], a.nz = hd[2], a.n = hd[3], a.H = hd[4], a.W = hd[5], a.M = hd[6];
    const bool has_color = hd[7] != 0;
    a.ox = pr[0], a.oy = pr[1], a.oz = pr[2], a.s = pr[3], a.min_weight = pr[4], a.step = pr[5], a.zmin = pr[6];
    a.invalid = pr[7];
    get(f, a.q, 16);
    const size_t V = (size_t)a.nx * a.ny * a.nz, P = (size_t)a.n * a.H * a.W;
    std::vector<float> pose((size_t)a.n * 12), tsdf(V), weight(V);
    std::vector<unsigned> color(has_color ? V : 0);
    get(f, pose.data(), pose.size());
    get(f, tsdf.data(), V);
    get(f, weight.data(), V);
    if (has_color) get(f, color.data(), V);
    fclose(f);
    const smx::RaycastLayout l = smx::raycast_layout(a.nx, a.ny, a.nz);
    a.bx = l.bx, a.by = l.by, a.bz = l.bz;
    // the brick bytes from their definition: RC_ANY, and RC_FREE over the brick's own voxels ...
    const size_t B = (size_t)l.bx * l.by * l.bz;
    std::vector<uint8_t> flags(B, smx::RC_FREE), occ(B, 0);
    for (int k = 0; k < a.nz; ++k)
        for (int j = 0; j < a.ny; ++j)
            for (int i = 0; i < a.nx; ++i) {
                const size_t v = ((size_t)k * a.ny + j) * a.nx + i;
                uint8_t &b = flags[((size_t)(k >> 3) * l.by + (j >> 3)) * l.bx + (i >> 3)];
                const bool ok = weight[v] >= a.min_weight;
                if (ok) b |= smx::RC_ANY;
                if (!(ok && tsdf[v] == 1.0f)) b &= (uint8_t)~smx::RC_FREE;
            }
    // ... then RC_FREE only with free upper neighbours
    size_t set = 0, free_bricks = 0;
    for (int k = 0; k < l.bz; ++k)
        for (int j = 0; j < l.by; ++j)
            for (int i = 0; i < l.bx; ++i) {
                unsigned free = smx::RC_FREE;
                for (int c = 0; c < 8; ++c) {
                    const int ni = i + (c & 1), nj = j + ((c >> 1) & 1), nk = k + (c >> 2);
                    if (ni < l.bx && nj < l.by && nk < l.bz) free &= flags[((size_t)nk * l.by + nj) * l.bx + ni];
                }
                const size_t b = ((size_t)k * l.by + j) * l.bx + i;
                occ[b] = (uint8_t)((flags[b] & smx::RC_ANY) | free);
                set += (occ[b] & smx::RC_ANY) != 0;
                free_bricks += free != 0;
            }
    std::vector<float> disp(P), depth(P), normals(3 * P), wout(P);
    std::vector<uint8_t> colors(has_color ? 3 * P : 0);
    a.tsdf = tsdf.data(), a.weight = weight.data(), a.color = has_color ? color.data() : nullptr;
    a.pose = pose.data();
    a.disp = disp.data(), a.depth = depth.data(), a.normals = normals.data(), a.out_weight = wout.data();
    a.colors = has_color ? colors.data() : nullptr;
    a.flags = flags.data(), a.occ = occ.data();
    for (int view = 0; view < a.n; ++view)
        for (int py = 0; py < a.H; ++py)
            for (int px = 0; px < a.W; ++px) smx::rc_pixel(a, px, py, view);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    fwrite(disp.data(), 4, P, o);
    fwrite(depth.data(), 4, P, o);
    fwrite(normals.data(), 4, 3 * P, o);
    fwrite(wout.data(), 4, P, o);
    if (has_color) fwrite(colors.data(), 1, 3 * P, o);
    fclose(o);
    printf("raycast-march pixels %zu bricks %zu set %zu free %zu\n", P, B, set, free_bricks);
    return 0;
}
