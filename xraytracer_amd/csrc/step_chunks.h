// step_chunks.h — block-owned slot chunks of the merged schedule's whole-wave phase.
//
// While a one-level merged render runs whole waves, its live slots are kept in chunks of at most
// kChunkSlots = 256 (one pass of a 4-wave block).  A chunk has two list segments and two counters of
// its own, and its slots never leave it while the phase lasts: after a pass the block's waves
// append the surviving slots to the chunk's other segment and meet at a barrier.  Within one launch
// a chunk is served by one block only, which runs a fixed number of passes over the chunks it owns
// and exits; no block waits for another, and a launch has no tail of late-starting waves, because
// the grid never exceeds the wave slots of the GPU (k_step_merged_chunks, step_merged.h).
//
// Chunks are numbered c = 8 j + x: x = c % 8 is the chunk's class, the residue of the partitions
// whose live lists were concatenated into it (k_chunks_build) and of the blocks that serve it, so a
// chunk's slots stay on one XCD as a partition's do (path_common.h part_iter); j counts the class's
// chunks.  A launch has m blocks per class, 8 m in all.  Class x with nx chunks deals them round
// robin: chunk j sits at position q = (j + rot) % nx and belongs to the class's block q % m, that is
// to block 8 (q % m) + x.  The host advances rot with every launch, so where a class has more
// chunks than blocks the double duty moves on.  Results never depend on any of it: a slot's path
// depends on the slot alone.
//
// These formulas are shared by the kernels and the host; what the host decides with them is
// host/step_chunks.cpp (plain host code, tests/cpp/step_chunks_kat.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define XRT_CHUNKS_FN __host__ __device__ inline
#else
#define XRT_CHUNKS_FN inline
#endif

namespace xrt {

constexpr uint32_t kChunkSlots = 256;        // live slots of a chunk at most: kBlock / 64 waves of 64
constexpr uint32_t kChunkClassBlocks = 128;  // blocks per class at most: 8 * 128 = 256 CUs * 4 resident blocks
constexpr uint32_t kChunkOwnMax = 32;        // chunks one block may own in a launch (the kernel's table)
// header words of the chunk buffer (k_chunks_build writes them): chunks per class, then live slots per class
constexpr uint32_t kChunkHdrWords = 16;

// chunks of class x among the chunks c < C of a dense numbering
XRT_CHUNKS_FN uint32_t chunk_class_count(uint32_t C, uint32_t x) { return (C + 7u - x) / 8u; }
// blocks per class of a launch whose fullest class has max_nx chunks
XRT_CHUNKS_FN uint32_t chunk_class_blocks(uint32_t max_nx) { return max_nx < kChunkClassBlocks ? max_nx : kChunkClassBlocks; }
// the block that owns chunk j of class x (nx chunks, m blocks per class) in the launch numbered rot
XRT_CHUNKS_FN uint32_t chunk_owner(uint32_t j, uint32_t x, uint32_t nx, uint32_t m, uint32_t rot) {
    return 8u * (((j + rot % nx) % nx) % m) + x;
}
// how many chunks the class's block bj (= block / 8) owns: the positions bj, bj + m, ... below nx
XRT_CHUNKS_FN uint32_t chunk_owned(uint32_t bj, uint32_t nx, uint32_t m) { return bj < nx && bj < m ? (nx - bj + m - 1u) / m : 0u; }
// ... and the t-th of them, as the chunk's index within its class
XRT_CHUNKS_FN uint32_t chunk_owned_at(uint32_t bj, uint32_t t, uint32_t nx, uint32_t m, uint32_t rot) {
    return (bj + t * m + nx - rot % nx) % nx;
}

// Dense arrays: class x holds the live entries of the partitions x, x + 8, ... one behind the other.
// Offset of partition p's entries in its class's array, given every partition's live count.
XRT_CHUNKS_FN uint32_t chunk_dense_offset(const uint32_t* part_live, uint32_t p) {
    uint32_t off = 0;
    for (uint32_t q = p & 7u; q < p; q += 8u) off += part_live[q];
    return off;
}
// live entries of class x
XRT_CHUNKS_FN uint32_t chunk_class_live(const uint32_t* part_live, uint32_t n_part, uint32_t x) {
    uint32_t tot = 0;
    for (uint32_t q = x; q < n_part; q += 8u) tot += part_live[q];
    return tot;
}
XRT_CHUNKS_FN uint32_t chunks_for(uint32_t live) { return (live + kChunkSlots - 1u) / kChunkSlots; }

// ---- host/step_chunks.cpp
// chunks per class the buffers must hold for n_part partitions of part_cap slots (every slot live)
uint32_t chunk_class_cap(uint32_t n_part, uint32_t part_cap);
// blocks of a launch over C chunks numbered densely: min(C, 1024) rounded up to a multiple of 8
uint32_t chunk_blocks(uint32_t C);
// Passes per block per launch: at most `cap` (XRT_CHUNK_PASSES), and so few that a launch is at most
// about a quarter of the visits a pixel is expected to need, spp * (max_depth + 2) / 2
uint32_t chunk_passes(uint32_t cap, uint32_t spp, uint32_t max_depth, uint32_t visits);
// What plan_render knows when it decides (the flags are xrt.h's XRT_FLAG_CHUNKS / NO_CHUNKS bits)
struct ChunkRule {
    bool one_level_merged;   // the merged schedule over pair passes: GI or Direct, not two-level, no moments
    bool starts_whole_waves; // step_merged_spw(P, n_slots) == 64
    bool interleaved;        // the render's slot map is the interleaved one by the library's own rule
    bool force, forbid;      // XRT_FLAG_CHUNKS, XRT_FLAG_NO_CHUNKS
    uint32_t visits_req, spw_req;   // the caller's visits_per_launch and slots_per_wave (0: unset)
    uint32_t spp, max_depth, visits;   // visits: per pass (RenderPlan::step_visits)
    uint32_t class_cap;      // chunk_class_cap of the render
    uint32_t pass_cap;       // XRT_CHUNK_PASSES
};
// passes per launch, or 0: the phase is not used
uint32_t chunk_plan(const ChunkRule& r);

}  // namespace xrt
