// tu_remap.hip -- bilinear remap (rectification) kernel (k_remap.h).
#include <stdint.h>

#include "k_remap.h"
#include "smx_launch.h"

namespace smx {

namespace {

template <typename T, bool REPLICATE, bool VEC>
void launch_t(dim3 grid, const RemapParams &p, hipStream_t s) {
    hipLaunchKernelGGL((k_remap<T, REPLICATE, VEC>), grid, dim3(REMAP_TX, REMAP_TY), 0, s, p);
}

template <typename T>
void launch_dtype(dim3 grid, const RemapParams &p, bool replicate, bool vec, hipStream_t s) {
    if (replicate) vec ? launch_t<T, true, true>(grid, p, s) : launch_t<T, true, false>(grid, p, s);
    else vec ? launch_t<T, false, true>(grid, p, s) : launch_t<T, false, false>(grid, p, s);
}

bool aligned(const void *ptr, uintptr_t a) { return ptr == nullptr || ((uintptr_t)ptr & (a - 1)) == 0; }

}  // namespace

void launch_remap_pairs(int n, int C, bool f32, int Hi, int Wi, int Ho, int Wo, const void *in_l, const void *in_r,
                        const int32_t *map_l, const int32_t *map_r, void *out_l, void *out_r, bool replicate,
                        float border_value, hipStream_t s) {
    RemapParams p;
    p.in[0] = in_l, p.in[1] = in_r;
    p.map[0] = map_l, p.map[1] = map_r;
    p.out[0] = out_l, p.out[1] = out_r;
    p.n = n, p.C = C, p.Hi = Hi, p.Wi = Wi, p.Ho = Ho, p.Wo = Wo;
    p.bval_f = border_value;
    p.bval_i = f32 ? 0 : (int)border_value;
    // REMAP_IPT images per thread; more when n is so large that gridDim.z would pass 65535
    const int views = in_r ? 2 : 1;
    // in 64 bits: n may be close to INT_MAX when the frames are tiny
    const long long nn = n;
    long long chunks = (nn + REMAP_IPT - 1) / REMAP_IPT;
    if (chunks > 16384) chunks = 16384;
    const long long ipt = (nn + chunks - 1) / chunks;
    p.ipt = (int)ipt;
    p.chunks = (int)((nn + ipt - 1) / ipt);
    const dim3 grid((unsigned)((Wo + REMAP_TX * REMAP_PX - 1) / (REMAP_TX * REMAP_PX)),
                    (unsigned)((Ho + REMAP_TY - 1) / REMAP_TY), (unsigned)(views * p.chunks));
    // the VEC form takes any width; it needs 8-byte aligned maps and element-aligned outputs (k_remap.h)
    const uintptr_t out_align = f32 ? 4 : 1;
    const bool vec = aligned(map_l, 8) && aligned(map_r, 8) && aligned(out_l, out_align) && aligned(out_r, out_align);
    if (f32) launch_dtype<float>(grid, p, replicate, vec, s);
    else launch_dtype<uint8_t>(grid, p, replicate, vec, s);
}

}  // namespace smx
