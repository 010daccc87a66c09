// Host-only harness of tests/test_workspace_layout_cpu.py: every workspace layout of stereo-depth_amd/csrc/smx_workspace.h,
// which the size queries and the launchers both read, against the properties a launcher relies on and against the size
// expressions the launchers used to write by hand.  It compiles the header's own lines and never calls the HIP runtime.
//
// For each layout, over the sweep of its arguments: every part starts on a multiple of 256 bytes, the first at 0; the
// parts ascend and their byte extents are disjoint; the last ends at or before `total`; `total` equals the former
// expression (the parent_* functions below, copied verbatim with their constants, never to be edited with the header);
// the derived counts a launcher takes from the layout equal the former ones.
//
// Output: a line per violation ("violation <what>: <inputs>", the first 60), then
//   "workspace-layout post <n> wls <n> sgm <n> reproject <n> voxel <n> tsdf_integrate <n> tsdf_extract <n> mesh <n>
//    violations <n>" with the number of layouts checked of each kind.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <initializer_list>

#include "smx_workspace.h"

using namespace smx;

static long violations = 0;
static void violation(const char *fmt, ...) {
    if (++violations > 60) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    printf("violation %s\n", buf);
}

// ---- the former size expressions, as the launchers had them ------------------------------------------------------------
namespace parent {
struct float2 { float x, y; };
constexpr int SCAN_ITEMS = 16;
constexpr int SCAN_TILE = 256 * SCAN_ITEMS;
constexpr int VOX_TILE = 4096;
constexpr int VM_COUNT = 16;
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t scan_block_sums(long L) { return (size_t)((L + SCAN_TILE - 1) / SCAN_TILE); }

static size_t post_workspace_bytes(int n, int H, int W) {
    const size_t px = (size_t)n * H * W;
    return 2 * align256(px * sizeof(int)) + align256((size_t)n * H * sizeof(int));
}

constexpr size_t WLS_ALIGN = 256;
static size_t wls_plane_bytes(int n, int H, int W) {
    return ((size_t)n * H * W * sizeof(float) + WLS_ALIGN - 1) / WLS_ALIGN * WLS_ALIGN;
}
static size_t wls_workspace_bytes(int n, int H, int W) { return 3 * wls_plane_bytes(n, H, W); }

constexpr size_t SGM_ALIGN = 256;
static size_t align_up(size_t v) { return (v + SGM_ALIGN - 1) / SGM_ALIGN * SGM_ALIGN; }
static int sgm_dpl(int D) { return D <= 64 ? 1 : D <= 128 ? 2 : 4; }
static int sgm_dp(int D) { const int k = sgm_dpl(D); return (D + k - 1) / k * k; }
static size_t sgm_workspace_bytes(int n, int H, int W, int D) {
    const size_t P = (size_t)n * H * W;
    size_t cen_l = 0;
    size_t cen_r = cen_l + align_up(P * 8);
    size_t S = cen_r + align_up(P * 8);
    size_t iR = S + align_up(P * sgm_dp(D) * 2);
    return iR + align_up(P * 2);
}

static size_t reproject_workspace_bytes(int n, int H) { return align256(2 * (size_t)n * H * sizeof(int)); }

struct Vox {
    size_t total;
    long max_tiles, Lc, Lf;
    int nb;
};
static Vox vox_layout(int n, int cap) {
    Vox l;
    l.max_tiles = ((long)cap + VOX_TILE - 1) / VOX_TILE + n;
    l.Lc = l.max_tiles * 256;
    l.Lf = (long)cap + 1;
    l.nb = (int)((std::max(l.Lc, l.Lf) + SCAN_TILE - 1) / SCAN_TILE);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    take(2 * (size_t)cap * sizeof(unsigned long long));
    take(2 * (size_t)cap * sizeof(int));
    take((size_t)l.Lc * sizeof(int));
    take((size_t)l.Lc * sizeof(int));
    take((size_t)l.Lf * sizeof(int));
    take((size_t)l.Lf * sizeof(int));
    take((size_t)l.Lf * sizeof(int));
    take((size_t)l.nb * sizeof(int));
    take(((size_t)n + 1) * sizeof(int));
    take(((size_t)n + 1) * sizeof(int));
    take(VM_COUNT * sizeof(int));
    l.total = at;
    return l;
}

static size_t tsdf_integrate_workspace_bytes(int n, int H, int W) {
    const size_t px = (size_t)n * H * W;
    return align256(px * sizeof(float2)) + align256(px * sizeof(unsigned));
}

static size_t tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
    (void)nx;
    const long rows = (long)ny * nz;
    return 2 * align256((size_t)rows * sizeof(int)) + align256(scan_block_sums(rows) * sizeof(int));
}

static size_t tsdf_triangles_workspace_bytes(int nx, int ny, int nz) {
    const size_t rows = (size_t)ny * nz;
    const int nch = (nx + 63) / 64;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t o = at; at += align256(bytes); return o; };
    take(rows * nx);
    take(rows * nch * sizeof(unsigned));
    take(3 * rows * sizeof(int));
    take(3 * rows * sizeof(int));
    take(scan_block_sums(3 * (long)rows) * sizeof(int));
    return at;
}
}  // namespace parent

// ---- the properties of one layout ----------------------------------------------------------------------------------------
static void check(const char *what, const char *args, std::initializer_list<WsPart> parts, size_t total, size_t expect) {
    size_t end = 0;
    int k = 0;
    for (const WsPart &p : parts) {
        if (p.offset % 256 != 0) violation("%s(%s): part %d starts at %zu, not a multiple of 256", what, args, k, p.offset);
        if (k == 0 && p.offset != 0) violation("%s(%s): the first part starts at %zu", what, args, p.offset);
        if (p.offset < end) violation("%s(%s): part %d at %zu starts inside its predecessor, which ends at %zu", what, args, k, p.offset, end);
        if (p.offset + p.bytes < p.offset) violation("%s(%s): part %d wraps", what, args, k);
        end = p.offset + p.bytes;
        ++k;
    }
    if (end > total) violation("%s(%s): the last part ends at %zu, past total %zu", what, args, end, total);
    if (total != expect) violation("%s(%s): total %zu, formerly %zu", what, args, total, expect);
}

int main() {
    long count[8] = {0};
    char args[96];
    const int dims[] = {1, 2, 3, 5, 37, 255, 256, 257, 1080, 32768};
    const int Ds[] = {1, 40, 64, 65, 128, 129, 256};
    for (int n : dims)
        for (int H : dims)
            for (int W : dims) {
                if ((long)n * H * W > (1L << 30)) continue;
                snprintf(args, sizeof args, "%d, %d, %d", n, H, W);
                const PostLayout p = post_layout(n, H, W);
                check("post_layout", args, {p.label, p.size, p.flags}, p.total, parent::post_workspace_bytes(n, H, W));
                const size_t px = (size_t)n * H * W;
                if (p.label.bytes != px * 4 || p.size.bytes != px * 4 || p.flags.bytes != (size_t)n * H * 4)
                    violation("post_layout(%s): a part's size", args);
                ++count[0];
                const WlsLayout w = wls_layout(n, H, W);
                check("wls_layout", args, {w.U, w.V, w.E}, w.total, parent::wls_workspace_bytes(n, H, W));
                if (w.U.bytes != px * 4 || w.V.bytes != px * 4 || w.E.bytes != px * 4) violation("wls_layout(%s): a plane's size", args);
                ++count[1];
                for (int D : Ds) {
                    snprintf(args, sizeof args, "%d, %d, %d, %d", n, H, W, D);
                    const SgmLayout s = sgm_layout(n, H, W, D);
                    check("sgm_layout", args, {s.cen_l, s.cen_r, s.S, s.iR}, s.total, parent::sgm_workspace_bytes(n, H, W, D));
                    if (s.Dp != parent::sgm_dp(D) || sgm_dpl(D) != parent::sgm_dpl(D) || s.Dp < D || s.Dp % sgm_dpl(D) != 0)
                        violation("sgm_layout(%s): Dp %d", args, s.Dp);
                    if (s.cen_l.bytes != px * 8 || s.cen_r.bytes != px * 8 || s.S.bytes != px * s.Dp * 2 || s.iR.bytes != px * 2)
                        violation("sgm_layout(%s): a part's size", args);
                    ++count[2];
                }
                snprintf(args, sizeof args, "%d, %d", n, H);
                const ReprojectLayout r = reproject_layout(n, H);
                check("reproject_layout", args, {r.rows}, r.total, parent::reproject_workspace_bytes(n, H));
                if (r.rows.bytes != 2 * (size_t)n * H * 4) violation("reproject_layout(%s): the rows' size", args);
                ++count[3];
                snprintf(args, sizeof args, "%d, %d, %d", n, H, W);
                const TsdfIntegrateLayout t = tsdf_integrate_layout(n, H, W);
                check("tsdf_integrate_layout", args, {t.meas, t.pcol}, t.total, parent::tsdf_integrate_workspace_bytes(n, H, W));
                if (t.meas.bytes != px * 8 || t.pcol.bytes != px * 4) violation("tsdf_integrate_layout(%s): a part's size", args);
                ++count[5];
            }
    for (int n : {1, 2, 65536})
        for (int cap : {1, 4095, 4096, 4097, 5000, 1 << 30}) {
            snprintf(args, sizeof args, "%d, %d", n, cap);
            const VoxLayout v = vox_layout(n, cap);
            const parent::Vox e = parent::vox_layout(n, cap);
            check("vox_layout", args, {v.keys, v.vals, v.counts, v.counts_scan, v.flag, v.pos, v.vcnt, v.block_sums, v.off,
                                       v.tile_base, v.meta}, v.total, e.total);
            if (v.max_tiles != e.max_tiles || v.Lc != e.Lc || v.Lf != e.Lf || v.nb != e.nb)
                violation("vox_layout(%s): max_tiles %ld Lc %ld Lf %ld nb %d", args, v.max_tiles, v.Lc, v.Lf, v.nb);
            // what the launcher and the kernels index: two buffers of cap keys / values, Lc histogram bins, Lf heads,
            // one block sum per scan tile of the longer of the two scans
            if (v.keys.bytes != 2 * (size_t)cap * 8 || v.vals.bytes != 2 * (size_t)cap * 4 || v.counts.bytes != (size_t)v.Lc * 4 ||
                v.counts_scan.bytes != (size_t)v.Lc * 4 || v.flag.bytes != (size_t)v.Lf * 4 || v.pos.bytes != (size_t)v.Lf * 4 ||
                v.vcnt.bytes != (size_t)v.Lf * 4 || v.block_sums.bytes < scan_block_sums(v.Lc) * 4 ||
                v.block_sums.bytes < scan_block_sums(v.Lf) * 4 || v.off.bytes != ((size_t)n + 1) * 4 ||
                v.tile_base.bytes != ((size_t)n + 1) * 4 || v.meta.bytes != VM_COUNT * 4)
                violation("vox_layout(%s): a part's size", args);
            ++count[4];
        }
    const int vol[] = {1, 8, 63, 64, 65, 70, 4096};
    for (int nx : vol)
        for (int ny : vol)
            for (int nz : vol) {
                if ((long)nx * ny * nz > (1L << 30)) continue;
                snprintf(args, sizeof args, "%d, %d, %d", nx, ny, nz);
                const size_t rows = (size_t)ny * nz;
                const TsdfExtractLayout x = tsdf_extract_layout(ny, nz);
                check("tsdf_extract_layout", args, {x.row_count, x.row_offset, x.block_sums}, x.total,
                      parent::tsdf_extract_workspace_bytes(nx, ny, nz));
                if (x.row_count.bytes != rows * 4 || x.row_offset.bytes != rows * 4 ||
                    x.block_sums.bytes != parent::scan_block_sums((long)rows) * 4)
                    violation("tsdf_extract_layout(%s): a part's size", args);
                ++count[6];
                const MeshLayout m = mesh_layout(nx, ny, nz);
                check("mesh_layout", args, {m.flags, m.chunk_first, m.counts, m.offsets, m.block_sums}, m.total,
                      parent::tsdf_triangles_workspace_bytes(nx, ny, nz));
                if (m.nch != (nx + 63) / 64 || m.flags.bytes != rows * nx || m.chunk_first.bytes != rows * m.nch * 4 ||
                    m.counts.bytes != 3 * rows * 4 || m.offsets.bytes != 3 * rows * 4 ||
                    m.block_sums.bytes != parent::scan_block_sums(3 * (long)rows) * 4)
                    violation("mesh_layout(%s): nch or a part's size", args);
                ++count[7];
            }
    if (SCAN_ITEMS != parent::SCAN_ITEMS || SCAN_TILE != parent::SCAN_TILE || VOX_TILE != parent::VOX_TILE ||
        VM_COUNT != parent::VM_COUNT)
        violation("a constant moved");
    printf("workspace-layout post %ld wls %ld sgm %ld reproject %ld voxel %ld tsdf_integrate %ld tsdf_extract %ld mesh %ld "
           "violations %ld\n", count[0], count[1], count[2], count[3], count[4], count[5], count[6], count[7], violations);
    return violations ? 1 : 0;
}
