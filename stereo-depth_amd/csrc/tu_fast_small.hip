// tu_fast_small.hip -- the latency shapes of the FAST_GRID kernel (few pairs in flight: 8-row bands, the
// disparity range split over the waves of a workgroup), the one-launch AUTO kernel built on it, and the
// dispatch of a FAST_GRID or filter launch to the translation unit of the band height its spec names.
#include "k_match_auto.h"
#include "k_match_filter.h"
#include "smx_launch.h"

namespace smx {

void launch_match_fast(const FastLaunch &fl, const MatchParams &p, int n, hipStream_t s) {
    if (fl.small) {
        if (fl.th == FA_TH_SMALL_TALL) {
            if (fl.pitch == 256) launch_match_fast_t<FA_TH_SMALL_TALL, 256, true>(fl, p, n, s);
            else launch_match_fast_t<FA_TH_SMALL_TALL, 320, true>(fl, p, n, s);
        } else if (fl.th == FA_TH_SMALL_MID) {
            if (fl.pitch == 256) launch_match_fast_t<FA_TH_SMALL_MID, 256, true>(fl, p, n, s);
            else launch_match_fast_t<FA_TH_SMALL_MID, 320, true>(fl, p, n, s);
        } else {
            if (fl.pitch == 256) launch_match_fast_t<FA_TH_SMALL, 256, true>(fl, p, n, s);
            else launch_match_fast_t<FA_TH_SMALL, 320, true>(fl, p, n, s);
        }
    } else if (fl.stack == FA_STACK) {
        launch_match_fast_stack(fl, p, n, s);
    } else if (fl.th == 27) {
        launch_match_fast_tall_27(fl, p, n, s);
    } else if (fl.th == 32) {
        launch_match_fast_tall_32(fl, p, n, s);
    } else {
        launch_match_fast_tall_24(fl, p, n, s);
    }
}

void launch_match_auto_small_tu(const AutoLaunch &al, const MatchParams &p, int n, hipStream_t s) { launch_match_auto_small(al, p, n, s); }

hipError_t match_auto_raise_caps() { return match_auto_raise_lds_caps(MATCH_AUTO_LDS_CAP); }

void launch_match_filter_tu(const FilterLaunch &fl, const MatchParams &p, const FilterParams &f, int n, hipStream_t s) {
    switch (fl.th) {
        case 24: launch_match_filter_24(fl, p, f, n, s); break;
        case 32: launch_match_filter_32(fl, p, f, n, s); break;
        default: launch_match_filter_27(fl, p, f, n, s); break;
    }
}

}  // namespace smx
