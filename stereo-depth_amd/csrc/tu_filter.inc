// tu_filter.inc -- one band height of the candidate-marking kernel (k_match_filter.h) per translation unit.
#include "k_match_filter.h"
#include "smx_launch.h"

#define SMX_TU_CAT2(a, b) a##b
#define SMX_TU_CAT(a, b) SMX_TU_CAT2(a, b)

namespace smx {
void SMX_TU_CAT(launch_match_filter_, SMX_TU_TH)(const FilterLaunch &fl, const MatchParams &p, const FilterParams &f, int n, hipStream_t s) {
    if (!fl.wide) launch_match_filter_t<SMX_TU_TH, 256>(fl.pk, p, f, n, s);
    else launch_match_filter_t<SMX_TU_TH, 320>(fl.pk, p, f, n, s);
}
}  // namespace smx
