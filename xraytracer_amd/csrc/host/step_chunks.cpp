// host/step_chunks.cpp — when a merged render keeps its whole-wave phase in block-owned chunks, and
// how its launches are sized (step_chunks.h has the ownership map the kernels share).  Plain host
// code: tests/cpp/step_chunks_kat.cpp compiles it on its own.
//
// Chunks change no result: a chunk's lists, counters and slots are touched by one block per launch,
// launches are ordered by their stream, and a slot's path depends on the slot alone.
#include "../step_chunks.h"

namespace xrt {

uint32_t chunk_class_cap(uint32_t n_part, uint32_t part_cap) {
    const uint32_t per_class = (n_part + 7u) / 8u;   // partitions of the fullest class
    return (uint32_t)(((uint64_t)per_class * part_cap + kChunkSlots - 1u) / kChunkSlots);
}

uint32_t chunk_blocks(uint32_t C) {
    const uint32_t most = 8u * kChunkClassBlocks;
    const uint32_t nb = (C < most ? C : most) + 7u;
    return nb & ~7u;
}

uint32_t chunk_passes(uint32_t cap, uint32_t spp, uint32_t max_depth, uint32_t visits) {
    if (visits == 0u) return 0u;
    const uint64_t quarter = (uint64_t)spp * ((uint64_t)max_depth + 2u) / (2ull * visits * 4ull);
    return (uint32_t)(quarter < cap ? quarter : cap);
}

uint32_t chunk_plan(const ChunkRule& r) {
    if (r.forbid || !r.one_level_merged || !r.starts_whole_waves) return 0u;
    // a block's table holds kChunkOwnMax chunks: larger renders keep the grouped schedule
    if (r.class_cap > kChunkOwnMax * kChunkClassBlocks) return 0u;
    if (r.force) return r.pass_cap >= 1u ? r.pass_cap : 1u;
    if (!r.interleaved || r.visits_req || r.spw_req) return 0u;
    // ... and, of those with two passes or more, only the renders that take the whole XRT_CHUNK_PASSES:
    // shorter launches amortise the scene copy over fewer passes and are not measured
    const uint32_t Q = chunk_passes(r.pass_cap, r.spp, r.max_depth, r.visits);
    return Q >= 2u && Q == r.pass_cap ? Q : 0u;
}

}  // namespace xrt
