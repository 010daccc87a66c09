// smx_status.h -- host-side status plumbing of the C ABI, shared by the engine (smx_engine.hip) and the engine-free
// entries (smx_maps.hip): the last-error text, HIP error mapping, device selection and the argument rules both apply.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cmath>

#include "../../include/stereo_mi355x.h"

namespace smx {

// Sets smx_last_error() (printf-style) and returns `code`; defined in smx_engine.hip.
int fail(int code, const char *fmt, ...);

#define SMX_HIP(call)                                                                        \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return smx::fail(e_ == hipErrorOutOfMemory ? SMX_ERR_OUT_OF_MEMORY : SMX_ERR_HIP, \
                             "%s failed: %s", #call, hipGetErrorString(e_));                 \
    } while (0)

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

inline bool ranges_overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
    if (!a || !b) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + bbytes && b0 < a0 + abytes;
}

inline int check_finite_marker(float invalid) {
    if (std::isfinite(invalid)) return SMX_OK;
    return fail(SMX_ERR_INVALID_ARG, "invalid_disparity must be finite (a NaN marker never compares equal), got %g",
                (double)invalid);
}

inline int check_lr_scalars(float max_diff, float invalid) {
    if (!(std::isfinite(max_diff) && max_diff >= 0.0f))
        return fail(SMX_ERR_INVALID_ARG, "max_diff must be finite and >= 0, got %g", (double)max_diff);
    return check_finite_marker(invalid);
}

}  // namespace smx
