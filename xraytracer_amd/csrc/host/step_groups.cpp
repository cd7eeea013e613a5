// host/step_groups.cpp — which partition groups the merged schedule's step launches run in
// (step_groups.h has the mapping the kernels share).  Plain host code: tests/cpp/
// step_groups_kat.cpp compiles it on its own.
//
// The groups change no result: a partition's list, counters and slots are touched by its own
// group's launches only, in the order one stream gives them.
#include "../step_groups.h"

namespace xrt {

bool step_groups_eligible(uint32_t n_part, uint32_t G) {
    if (G == 1u) return true;
    return G >= 1u && G <= kMaxStepGroups && n_part % 8u == 0u && n_part >= 8u * G;
}

uint32_t step_groups_for(uint32_t n_part, uint32_t want) {
    uint32_t G = want < kMaxStepGroups ? want : kMaxStepGroups;
    while (G > 1u && !step_groups_eligible(n_part, G)) --G;
    return G < 1u ? 1u : G;
}

}  // namespace xrt
