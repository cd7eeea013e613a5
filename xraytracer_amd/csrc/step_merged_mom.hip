// step_merged_mom.hip — the moments builds of the merged step kernels (step_merged.h, MOM) and
// their launch, which launch_step_merged (step_merged.hip) forwards a variance render to.
#include "step_merged.h"

namespace xrt {

hipError_t launch_step_merged_mom(const KParams& P, const KParams* dP, const StepObjs& SO, const uint32_t* list,
                                  const uint32_t* count, uint32_t* out, uint32_t* out_count, uint32_t* zero,
                                  float2* mom, uint32_t visits, uint64_t live, uint32_t live_part_max,
                                  uint32_t groups, uint32_t group, hipStream_t st) {
    return launch_step_merged_as<true>(P, dP, SO, list, count, out, out_count, zero, mom, visits, live, live_part_max, groups,
                                       group, st);
}

}  // namespace xrt
