// tu_median.hip -- image-guided weighted median kernel (k_median.h).
#include <string.h>

#include "k_median.h"
#include "smx_launch.h"

namespace smx {

// k_median keeps no state between phases: the call needs no workspace
size_t median_workspace_bytes(int, int, int) { return 0; }

namespace {

template <int SPL>
void launch_spl(unsigned grid, const float *in, const float *holes, const float *guide, float *out, int H, int W,
                int radius, float invalid, size_t tiles, int tiles_w, int tiles_per_map, const MedTables &tab,
                hipStream_t s) {
    hipLaunchKernelGGL((k_median<SPL>), dim3(grid), dim3(MED_THREADS), 0, s, in, holes, guide, out, H, W, radius,
                       invalid, tiles, tiles_w, tiles_per_map, tab);
}

}  // namespace

void launch_weighted_median(int n, int H, int W, const float *in, const float *holes, const float *guide, float *out,
                            int radius, const uint16_t *range, const uint16_t *spatial, float invalid, hipStream_t s) {
    MedTables tab;
    memset(&tab, 0, sizeof tab);
    memcpy(tab.range, range, sizeof tab.range);
    memcpy(tab.spatial, spatial, (size_t)(radius + 1) * (radius + 1) * sizeof(uint16_t));
    const int tiles_w = (W + MED_TW - 1) / MED_TW;
    const int tiles_per_map = ((H + MED_TH - 1) / MED_TH) * tiles_w;
    const size_t tiles = (size_t)n * tiles_per_map;
    const unsigned grid = (unsigned)(tiles < ((size_t)1 << 20) ? tiles : ((size_t)1 << 20));   // grid-stride beyond
    // samples per lane: the smallest instantiated bucket that holds the (2 radius + 1)^2 window on 64 lanes
    const int need = ((2 * radius + 1) * (2 * radius + 1) + 63) / 64;
#define SMX_MED_SPL(N) launch_spl<N>(grid, in, holes, guide, out, H, W, radius, invalid, tiles, tiles_w, tiles_per_map, tab, s)
    if (need <= 1) SMX_MED_SPL(1);
    else if (need <= 2) SMX_MED_SPL(2);
    else if (need <= 4) SMX_MED_SPL(4);
    else if (need <= 6) SMX_MED_SPL(6);
    else if (need <= 8) SMX_MED_SPL(8);
    else if (need <= 12) SMX_MED_SPL(12);
    else SMX_MED_SPL(16);
#undef SMX_MED_SPL
}

}  // namespace smx
