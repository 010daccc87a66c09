// tu_fast_tall.inc -- one band height of the tall-band FAST_GRID kernel per translation unit
// (SMX_TU_TH is defined by the including tu_fast_tall_NN.hip): 12 instantiations of the fully unrolled
// march each, compiled in parallel.
#include "k_match_fast.h"
#include "smx_launch.h"

#define SMX_TU_CAT2(a, b) a##b
#define SMX_TU_CAT(a, b) SMX_TU_CAT2(a, b)

namespace smx {
void SMX_TU_CAT(launch_match_fast_tall_, SMX_TU_TH)(const FastLaunch &fl, const MatchParams &p, int n, hipStream_t s) {
    launch_match_fast_tall<SMX_TU_TH>(fl, p, n, s);
}
}  // namespace smx
