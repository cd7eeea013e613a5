// step_sources.h — where a launch of the merged step kernels finds the slots it runs
// (step_merged_body, step_merged.h).  A source is the kernel's own arguments under their names, built
// by the kernel and passed to the body by value.  The block's place in its lists is a Pass, a local
// of the body beside the source: PartIter or ChunkIter (path_common.h), handed to the sources' methods
// by value where they only read it.  The body runs passes, `for (base = first; next_pass; base +=
// stride)`: a pass is up to per = (kBlock / 64) * SPW entries of one list from `base` on, the block's
// share of it.  What every source provides, every value block-uniform:
//   layout_ok<...>()      the kernel layouts the source serves (a static assertion of the body)
//   clock_tag()           the tag of the wave's clock record (experiment builds, WaveClock)
//   clear(P)              clear this launch's share of the next-next round's counters
//   begin(P, per, arg)    the Pass before the first pass; arg: the body's visits argument as passed
//   visits(arg)           the visits per pass in that argument (the chunks pack their passes above)
//   first(ps), stride(ps) the block's first entry and its step from pass to pass
//   next_pass(ps, base)   is there a pass at `base` (the chunks: pick the next chunk); false: none left
//   n_in(ps)              entries of the list that pass reads
//   slot(P, ps, i)        the slot at entry i < n_in(ps)
//   append(P, ps, ...)    a survivor of the pass onto the list the next launch (or pass) reads;
//                         must be called by every thread of the block
//   pass_end()            after the pass's last write
//   finish(P, ps)         by the block's first thread after the last pass: what the launch leaves
//                         for the host's poll
// The shape is what the compiler keeps every kernel's instruction stream for: the Pass
// as a member of the source, or taken by reference where by value would do, reorders instructions of
// the every-partition kernels.
// Device code only.
#pragma once
#include "merged.h"
#include "path_common.h"

namespace xrt {

// The partition lists (path_common.h, PartIter): a pass is a stride over the block's partition, a
// survivor goes to that partition's list of the next round, one atomic per wave, and the host polls
// the counters the appends leave.
struct PartSlots {
    const uint32_t *list, *count;
    uint32_t *out, *out_count, *zero_count;
    using Pass = PartIter;
    __device__ __forceinline__ uint32_t first(const Pass ps) const { return ps.first; }
    __device__ __forceinline__ uint32_t stride(const Pass ps) const { return ps.stride; }
    __device__ __forceinline__ bool next_pass(const Pass ps, uint32_t base) const { return base < ps.n; }
    __device__ __forceinline__ uint32_t n_in(const Pass ps) const { return ps.n; }
    __device__ __forceinline__ uint32_t slot(const KParams& P, const Pass ps, uint32_t i) const {
        return list[ps.p * P.part_cap + i];
    }
    __device__ __forceinline__ void append(const KParams& P, const Pass ps, bool want, uint32_t s, int lane, int) const {
        wave_append(want, s, out + ps.p * P.part_cap, out_count + ps.p, lane);
    }
    __device__ __forceinline__ void pass_end() const {}
    __device__ __forceinline__ uint32_t visits(uint32_t arg) const { return arg; }
    __device__ __forceinline__ void finish(const KParams&, const Pass) const {}
};

// Every partition (k_step_merged): block b serves partition b % n_part.
struct EveryPart : PartSlots {
    template <int SPW, int G, bool LANE, bool BVH, bool MOM>
    static constexpr bool layout_ok() { return true; }
    __device__ __forceinline__ uint32_t clock_tag() const { return ~0u; }
    __device__ __forceinline__ void clear(const KParams& P) const { zero_parts(P, zero_count); }
    __device__ __forceinline__ Pass begin(const KParams& P, uint32_t per_block, uint32_t) const {
        return part_iter(P, count, per_block);
    }
};

// One partition group of a round (k_step_merged_group; step_groups.h, grp: step_group_arg): its
// partitions' lists and counters only — another group's launch of the round before may still be
// appending to its own.  Whole waves of one-level scenes.
struct OneGroup : PartSlots {
    uint32_t grp;
    template <int SPW, int G, bool LANE, bool BVH, bool MOM>
    static constexpr bool layout_ok() { return SPW == 64 && G == 1 && !LANE && !BVH; }
    __device__ __forceinline__ uint32_t clock_tag() const { return grp; }
    __device__ __forceinline__ void clear(const KParams&) const { zero_parts(zero_count, grp); }
    __device__ __forceinline__ Pass begin(const KParams&, uint32_t per_block, uint32_t) const {
        return part_iter(count, per_block, grp);
    }
};

// Experiment builds (XRT_PHASE_CLOCK, tools/wave_timeline.py --chunks): lane 0 of every wave of the
// chunk kernel records the wall clock before and after each barrier of a pass end, with the
// survivors the wave counted in that pass; wave_clock_dump writes the records behind the waves'.
// kind 0: the barrier of the append (the waves' counts meet), 1: the barrier that ends the pass.
#if XRT_PHASE_CLOCK
constexpr uint32_t kPassClockCap = 1u << 19;
struct PassClockRec {
    uint32_t block, wave_kind, n, pad;   // wave_kind: wave of the block | kind << 8
    unsigned long long before, after;
};
static __device__ PassClockRec g_pass_clock[kPassClockCap];
static __device__ unsigned int g_pass_clock_n;
__device__ __forceinline__ uint32_t pass_clock_before(uint32_t kind, uint32_t n, int tid) {
    uint32_t idx = kPassClockCap;
    if ((tid & 63) == 0) {
        idx = atomicAdd(&g_pass_clock_n, 1u);
        if (idx < kPassClockCap) {
            g_pass_clock[idx].block = blockIdx.x, g_pass_clock[idx].wave_kind = (uint32_t)(tid >> 6) | kind << 8;
            g_pass_clock[idx].n = n, g_pass_clock[idx].pad = 0;
            g_pass_clock[idx].before = wall_clock64();
        }
    }
    return idx;
}
__device__ __forceinline__ void pass_clock_after(uint32_t idx) {
    if (idx < kPassClockCap) g_pass_clock[idx].after = wall_clock64();
}
#endif

// The chunk phase (k_step_merged_chunks; step_chunks.h): the chunks this block owns in the launch
// numbered rot, over ChunkIter and its steps (path_common.h).  A pass runs one chunk: its survivors go
// to the chunk's other segment, and the block meets at a barrier before the next.  Whole waves of
// one-level scenes, plain renders.  The kernel hands the body visits | passes << 8 for `visits` (both
// at most 255, launch_step_merged_chunks): begin and visits take them apart.  (Passed as a member of
// their own the passes cost every chunk kernel its instruction stream, DESIGN.md.)
constexpr uint32_t kChunkClockTag = 0xFFFFFFFEu;   // the chunk kernel's waves in the wave clock records (~0: every partition)
struct OwnedChunks {
    const uint32_t* hdr;   // k_chunks_build's header (chunks per class)
    uint32_t *cnt, *seg;   // the chunks' counters and segments
    uint32_t *live_count, *zero_count;
    uint32_t rot;
    using Pass = ChunkIter;
    template <int SPW, int G, bool LANE, bool BVH, bool MOM>
    static constexpr bool layout_ok() { return SPW == 64 && G == 1 && !LANE && !BVH && !MOM; }
    __device__ __forceinline__ uint32_t clock_tag() const { return kChunkClockTag; }
    __device__ __forceinline__ void clear(const KParams& P) const { zero_parts(P, zero_count); }
    __device__ __forceinline__ Pass begin(const KParams&, uint32_t, uint32_t arg) const {
        return chunk_iter(hdr, cnt, seg, rot, arg >> 8);
    }
    __device__ __forceinline__ uint32_t visits(uint32_t arg) const { return arg & 255u; }
    __device__ __forceinline__ uint32_t first(const Pass&) const { return 0u; }
    __device__ __forceinline__ uint32_t stride(const Pass&) const { return 0u; }
    __device__ __forceinline__ bool next_pass(Pass& K, uint32_t) const { return chunk_next(K); }
    __device__ __forceinline__ uint32_t n_in(const Pass& K) const { return K.n; }
    __device__ __forceinline__ uint32_t slot(const KParams&, const Pass& K, uint32_t i) const {
        return glb<gu32>(K.seg + (size_t)(2u * K.c + K.h) * kChunkSlots)[i];
    }
    __device__ __forceinline__ void append(const KParams&, Pass& K, bool want, uint32_t s, int lane, int tid) const {
#if XRT_PHASE_CLOCK
        const uint32_t ck = pass_clock_before(0u, (uint32_t)__popcll(__ballot(want)), tid);
#endif
        chunk_append(K, want, s, lane, tid);
#if XRT_PHASE_CLOCK
        pass_clock_after(ck);
#endif
    }
    __device__ __forceinline__ void pass_end() const {
#if XRT_PHASE_CLOCK
        const uint32_t ck = pass_clock_before(1u, 0u, (int)threadIdx.x);
#endif
        chunk_pass_end();
#if XRT_PHASE_CLOCK
        pass_clock_after(ck);
#endif
    }
    // the live slots the block's chunks are left with, summed over the launch's blocks
    __device__ __forceinline__ void finish(const KParams& P, const Pass& K) const {
        const uint32_t left = chunk_live(K);
        if (left) atomicAdd(live_count + blockIdx.x % P.n_part, left);
    }
};

}  // namespace xrt
