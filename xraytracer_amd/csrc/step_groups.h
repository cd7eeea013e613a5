// step_groups.h — partition groups of the merged schedule's step launches.
//
// A slot's path depends on nothing outside the slot and the live lists are per partition, so the
// step launches of disjoint sets of partitions need not wait for each other: the partitions are
// dealt to G groups in whole octets, group(p) = (p / 8) % G, and every group's launches run on a
// stream of their own (run_fused, api_render.cpp).  Interleaved octets, not image bands, so all
// groups run out of live pixels at about the same time; whole octets, so a block's partition
// still has p % 8 == blockIdx % 8 and a partition's slots stay on one XCD (path_common.h
// part_iter).  The two formulas are shared by the kernels and the host; what the host decides
// with them is host/step_groups.cpp (plain host code, tests/cpp/step_groups_kat.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define XRT_GROUPS_FN __host__ __device__ inline
#else
#define XRT_GROUPS_FN inline
#endif

namespace xrt {

constexpr uint32_t kMaxStepGroups = 3;   // with the context's own stream: 4 streams, the process's hardware queues

// partitions of group g of G over n_part partitions (a multiple of 8): its octets g, g + G, ...
XRT_GROUPS_FN uint32_t step_group_parts(uint32_t n_part, uint32_t G, uint32_t g) {
    const uint32_t oct = n_part / 8u;
    return g < oct ? 8u * ((oct - g + G - 1u) / G) : 0u;
}
// the partition that block-local partition lp of group g serves; G = 1: lp itself
XRT_GROUPS_FN uint32_t step_group_part(uint32_t G, uint32_t g, uint32_t lp) {
    return ((lp >> 3) * G + g) * 8u + (lp & 7u);
}
// the group of partition p
XRT_GROUPS_FN uint32_t step_group_of(uint32_t G, uint32_t p) { return (p >> 3) % G; }

// A launch's group as one kernel argument: g in bits 0..3, G in bits 4..7, the partitions the
// launch serves above (G = 1: all n_part of them, of any count)
XRT_GROUPS_FN uint32_t step_group_arg(uint32_t n_part, uint32_t G, uint32_t g) {
    return g | (G << 4) | ((G > 1u ? step_group_parts(n_part, G, g) : n_part) << 8);
}

// host/step_groups.cpp.  Eligibility: G groups (1..kMaxStepGroups) over n_part partitions need
// whole octets and at least one per group, n_part % 8 == 0 and n_part >= 8 * G; one group always is.
bool step_groups_eligible(uint32_t n_part, uint32_t G);
// the groups a render of n_part partitions runs in when `want` are asked for: the most, up to
// `want`, that are eligible
uint32_t step_groups_for(uint32_t n_part, uint32_t want);

}  // namespace xrt
