// tu_exact.hip -- the exact-order aggregation kernels (k_match_exact.h: any radii; k_match_exact2.h: default
// radii, register-tiled; its disparity-split, sparse-candidate and capture variants): from launch spec to instantiation.
#include "k_match_exact.h"
#include "k_match_exact2.h"
#include "smx_launch.h"

namespace smx {

void launch_exact(const ExactLaunch &x, const MatchParams &p, int n, hipStream_t s) {
    if (x.kernel == EXACT_TILED) {      // default radii: register-tiled kernel (4x2 outputs per thread, 64-bit LDS reads)
        const dim3 grid((p.w + E2_TW - 1) / E2_TW, (p.h + E2_TH - 1) / E2_TH, n * x.split);
        if (x.split > 1) {
            // few pairs in flight: slices of the disparity range run as separate workgroups, merged afterwards by a merge
            // launch, not by a tile's last slice (p.tickets == nullptr; k_match_auto.h uses that): measured 5 - 8 us slower
            // per frame here (write-through records, the merge on the tail of the slowest tile)
            if (x.rows_per_thread == 4) hipLaunchKernelGGL((k_match_exact2<true, 4>), grid, dim3(E2K<4>::THREADS), x.lds_bytes, s, p);
            else hipLaunchKernelGGL((k_match_exact2<true, 2>), grid, dim3(E2K<2>::THREADS), x.lds_bytes, s, p);
            hipLaunchKernelGGL(k_match_merge<0>, dim3((unsigned)(((size_t)p.h * p.w + 255) / 256), 1, n), dim3(256), 0, s, p);
        } else {
            hipLaunchKernelGGL((k_match_exact2<false, 4>), grid, dim3(E2K<4>::THREADS), x.lds_bytes, s, p);
        }
        return;
    }
    const dim3 grid((p.w + EX_TW - 1) / EX_TW, (p.h + EX_TH - 1) / EX_TH, n);
    if (x.kernel == EXACT_GENERIC_VOLUME) hipLaunchKernelGGL((k_match_exact<-1, -1, -1, -1, true>), grid, dim3(256), x.lds_bytes, s, p);
    else hipLaunchKernelGGL((k_match_exact<-1, -1, -1, -1, false>), grid, dim3(256), x.lds_bytes, s, p);
}

// dmin > 0 (capture route), exact-order variant: the lookups of step 6 from the arg-max the kernel above wrote
void launch_exact2_capture(const ExactCaptureLaunch &x, const MatchParams &p, int n, hipStream_t s) {
    const dim3 grid((p.w + E2_TW - 1) / E2_TW, (p.h + E2_TH - 1) / E2_TH, n * x.split);
    if (x.rows_per_thread == 2) hipLaunchKernelGGL(k_match_exact2_capture<2>, grid, dim3(E2K<2>::THREADS), x.lds_bytes, s, p);
    else hipLaunchKernelGGL(k_match_exact2_capture<4>, grid, dim3(E2K<4>::THREADS), x.lds_bytes, s, p);
}

void launch_exact2_sparse(const MatchParams &p, int n, unsigned *cand, int cw, const int *range_flags, unsigned *stats_dev,
                          unsigned long long *stats_host, unsigned seq, hipStream_t s) {
    const dim3 grid((p.w + E2_TW - 1) / E2_TW, (p.h + E2_TH - 1) / E2_TH, n);
    hipLaunchKernelGGL(k_match_exact2_sparse<4>, grid, dim3(E2K<4>::THREADS), exact2_sparse_lds_bytes(p.nd_chunk), s, p, cand, cw, range_flags,
                       SparseStats{stats_dev, stats_host, seq});
}

// Dynamic LDS above 64 KB must be requested per kernel (and device).
hipError_t exact_raise_lds_caps(int cap_bytes) {
    const void *fns[] = {reinterpret_cast<const void *>(&k_match_exact2<false, 4>), reinterpret_cast<const void *>(&k_match_exact2<true, 4>),
                         reinterpret_cast<const void *>(&k_match_exact2<true, 2>),
                         reinterpret_cast<const void *>(&k_match_exact2_capture<4>), reinterpret_cast<const void *>(&k_match_exact2_capture<2>),
                         reinterpret_cast<const void *>(&k_match_exact2_sparse<4>)};
    for (const void *f : fns) {
        hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, cap_bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace smx
