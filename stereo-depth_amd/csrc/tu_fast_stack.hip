// tu_fast_stack.hip -- the stacked bands of the tall-band FAST_GRID kernel (k_match_fast.h: FA_STACK): 2 x 24 output rows
// for 70 marched ones, sparse form, pitch 256, compiled for two waves per SIMD.
//
// Register budget.  A workgroup's 68.6 KB tile fits a CU twice, so every SIMD holds two of this kernel's waves.  Step 6 of
// the other stream lane (k_refine_auto_v<2>: 117 registers, allocated in blocks of 8 as 120) has to fit beside them in the
// 512 registers of a SIMD: 2 x 192 + 120 = 504.  The kernel takes 182 (K <= 2, box sums from prefix sums) / 184 (K = 4) /
// 188 (K = 8) registers (profiles/r08_kernel_resources.txt), allocated as 192 at most, and is held to 192 (amdgpu_num_vgpr
// through SMX_FA_NUM_VGPR).
// The march of 72 row steps only stays in registers when it is fully unrolled (build.py: PER_FILE_FLAGS); build.py
// refuses this unit if an instantiation reports scratch or a spill.
#define SMX_FA_OCC 2
#define SMX_FA_NUM_VGPR 192
#include "k_match_fast.h"
#include "smx_launch.h"

namespace smx {
constexpr int REFINE_AUTO_V2_VGPRS = 120;      // allocation of k_refine_auto_v<2> (profiles/r05_kernel_resources.txt)
static_assert(2 * SMX_FA_NUM_VGPR + REFINE_AUTO_V2_VGPRS <= 512, "two stacked aggregation waves and one step-6 wave share a SIMD");

void launch_match_fast_stack(const FastLaunch &fl, const MatchParams &p, int n, hipStream_t s) {
    launch_match_fast_stacked<256>(fl, p, n, s);
}
hipError_t fast_stack_raise_caps() { return fast_stacked_raise_lds_caps<256>(); }
}  // namespace smx
