// chunk_lists.hip — the lists of the merged schedule's chunk phase (step_chunks.h; the phase's step
// kernel is k_step_merged_chunks, step_merged.h): the chunks of a render from its seeded partition
// lists, and back onto the partition lists when the phase ends.
#include "launch.h"
#include "path_common.h"

namespace xrt {

// The chunks of a render from its partition lists, in two launches of one block per partition.
// k_chunks_count: the partition's live entries that are not ST_DONE (k_camlist's retired pixels stay
// on the seeded lists; no chunk holds them).
__global__ __launch_bounds__(kBlock) void k_chunks_count(KParams P, const uint32_t* __restrict__ list,
                                                         const uint32_t* __restrict__ count, uint32_t* part_live) {
    __shared__ uint32_t red[kBlock / 64];
    const uint32_t p = blockIdx.x, n = min(count[p], P.part_cap);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t keep = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) keep += (P.state[list[(size_t)p * P.part_cap + i]] & ST_DONE) ? 0u : 1u;
    for (int off = 32; off > 0; off >>= 1) keep += __shfl_down(keep, off);
    if (lane == 0) red[wv] = keep;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t tot = 0;
        for (int w = 0; w < kBlock / 64; ++w) tot += red[w];
        part_live[p] = tot;
    }
}
// k_chunks_build: class x = p % 8 concatenates those entries of the partitions x, x + 8, ... into one
// dense array, in list order, cut into chunks c = 8 j + x of kChunkSlots entries (segment 0).  The
// class's first partition also writes its header words and every counter of its chunks, up to the
// class_cap chunks the buffers hold.  The host has cleared header and counters: a class without a
// partition has no chunk.
__global__ __launch_bounds__(kBlock) void k_chunks_build(KParams P, const uint32_t* __restrict__ list,
                                                         const uint32_t* __restrict__ count,
                                                         const uint32_t* __restrict__ part_live, uint32_t* hdr, uint32_t* cnt,
                                                         uint32_t* seg, uint32_t class_cap) {
    __shared__ uint32_t wc[kBlock / 64];
    const uint32_t p = blockIdx.x, x = p & 7u, n = min(count[p], P.part_cap);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t run = chunk_dense_offset(part_live, p);
    for (uint32_t base = 0; base < n; base += kBlock) {
        const uint32_t i = base + (uint32_t)tid;
        const uint32_t s = i < n ? list[(size_t)p * P.part_cap + i] : 0u;
        const bool keep = i < n && !(P.state[s] & ST_DONE);
        const uint64_t m = __ballot(keep);
        if (lane == 0) wc[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < kBlock / 64; ++w) before += w < wv ? wc[w] : 0u, total += wc[w];
        const uint32_t pos = run + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        const uint32_t j = pos / kChunkSlots;
        if (keep && j < class_cap) seg[(size_t)(2u * (8u * j + x)) * kChunkSlots + pos % kChunkSlots] = s;
        run += total;
        __syncthreads();
    }
    if (p < 8u) {
        const uint32_t tot = chunk_class_live(part_live, P.n_part, x);
        if (tid == 0) hdr[x] = min(chunks_for(tot), class_cap), hdr[8u + x] = tot;
        for (uint32_t j = tid; j < class_cap; j += kBlock) {
            const uint32_t lo = j * kChunkSlots;
            cnt[2u * (8u * j + x)] = tot > lo ? min(kChunkSlots, tot - lo) : 0u;
            cnt[2u * (8u * j + x) + 1u] = 0u;
        }
    }
}
// k_chunks_scatter ends the phase: every chunk's live slots onto the partition lists the grouped
// schedule goes on with, slot s on the list of its partition s / part_cap (k_seed's), whose counters
// the host has cleared.  One block per chunk; a wave appends once per partition its slots come from.
__global__ __launch_bounds__(kBlock) void k_chunks_scatter(KParams P, const uint32_t* __restrict__ cnt,
                                                           const uint32_t* __restrict__ seg, uint32_t* out, uint32_t* out_count) {
    const uint32_t c = blockIdx.x, n0 = cnt[2u * c], n1 = cnt[2u * c + 1u];
    const uint32_t h = n0 ? 0u : 1u, n = min(n0 | n1, kChunkSlots);
    const int lane = threadIdx.x & 63;
    const bool have = threadIdx.x < n;
    const uint32_t s = have ? seg[(size_t)(2u * c + h) * kChunkSlots + threadIdx.x] : 0u;
    const uint32_t p = min(s / P.part_cap, P.n_part - 1u);
    uint64_t todo = __ballot(have);
    while (todo) {
        const uint32_t pl = (uint32_t)__builtin_amdgcn_readlane((int)p, __builtin_ctzll(todo));
        const bool mine = have && p == pl;
        wave_append(mine, s, out + (size_t)pl * P.part_cap, out_count + pl, lane);
        todo &= ~__ballot(mine);
    }
}

hipError_t launch_chunks_build(const KParams& P, const ChunkBufs& B, const uint32_t* list, const uint32_t* count,
                               hipStream_t st) {
    hipLaunchKernelGGL(k_chunks_count, dim3(P.n_part), dim3(kBlock), 0, st, P, list, count, B.part_live);
    hipLaunchKernelGGL(k_chunks_build, dim3(P.n_part), dim3(kBlock), 0, st, P, list, count, B.part_live, B.hdr, B.cnt, B.seg,
                       B.class_cap);
    return hipGetLastError();
}

hipError_t launch_chunks_scatter(const KParams& P, const ChunkBufs& B, uint32_t* out, uint32_t* out_count, hipStream_t st) {
    hipLaunchKernelGGL(k_chunks_scatter, dim3(8u * B.class_cap), dim3(kBlock), 0, st, P, B.cnt, B.seg, out, out_count);
    return hipGetLastError();
}

}  // namespace xrt
