// progressive.hip — the kernels of a progressive session (xrt_progressive_*, api_progressive.cpp) around
// the path work of a pass, which is every schedule's own: k_resume in k_seed's place before each pass,
// k_progress_finish in k_finish's after it, and k_progress_frame, the frame of the samples so far.
//
// A slot's stream, its counters and its moments record are absolute (ring, rng_c, rng_g, c_*, mom), the
// kernels add a pixel's accepted samples to its running sum in sample order, and the slot -> pixel map
// does not depend on the sample count: a pass that starts from what the last one left continues the
// one-shot render, bit for bit.  What a one-shot render does around that — reset the slots (k_seed),
// divide the sums in place (k_finish) — is what these kernels leave out.
#include "launch.h"
#include "path_common.h"

namespace xrt {

// ================================================================== k_resume ====
// Every slot back on the first list, between samples (ST_REGEN, no sample of this pass finished), and
// the partition counters as k_seed leaves them, but nothing requested: the rings are twisted here.
// The step kernels start a launch on the precondition that a live slot has at least rng_keep words
// ahead; the pass before ended each slot without asking for its next block (a finished slot asks for
// nothing), and this pass's plan may keep more words than the last one's.  A slot short of rng_keep
// gets its next block now, by its wave: legal as in a step launch, rng_keep <= kMT, so the new block
// overwrites drawn words only.  The slots twisted are counted in stats[kStatsResume].
__global__ __launch_bounds__(kBlock) void k_resume(KParams P, uint32_t* list, uint32_t* count, uint32_t* count_other,
                                                    uint32_t* req_count) {
    __shared__ __attribute__((aligned(16))) uint32_t rbuf[kBlock / 64][kMT];   // wave_refill staging
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    const bool valid = s < P.n_slots;
    uint32_t g = 0;
    bool want = false;
    if (valid) {
        g = P.rng_g[s];
        want = g - P.rng_c[s] < P.rng_keep;
        P.state[s] = ST_REGEN;
        P.sample_k[s] = 0;
        P.depth[s] = 0;
        P.occ[s] = 0;
        list[s] = s;   // partition p = s / part_cap starts at p * part_cap: identity
    }
    if (blockIdx.x == 0) {
        for (uint32_t p = threadIdx.x; p < P.n_part; p += kBlock) {
            const uint32_t lo = p * P.part_cap;
            count[p] = lo < P.n_slots ? min(P.part_cap, P.n_slots - lo) : 0u;
            count_other[p] = 0;
            req_count[p] = 0;
            req_count[kMaxParts + p] = 0;
        }
    }
    const uint64_t m = __ballot(want);
    if (lane == 0 && m) atomicAdd(P.stats + kStatsResume, (unsigned long long)__popcll(m));
    wave_refill(P, want, valid ? s : 0u, g, lane, rbuf[wv]);
}

// ========================================================= k_progress_finish ====
// k_finish without the division: the accumulator stays the pixels' running sums.
__global__ __launch_bounds__(kBlock) void k_progress_finish(KParams P) {
    SlotCounters cnt;
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < P.n_slots; s += gridDim.x * kBlock) cnt.add(P, s);
    cnt.reduce(P);
}

// ========================================================== k_progress_frame ====
// The frame of the spp_done = P.spp samples so far, out of place: rgb = acc / n for the shard's pixels
// (P.fb is the accumulator) and, with mom and var, the variance plane — k_finish's and k_finish_var's
// arithmetic (frame_mean, frame_variance).  The caller has cleared both outputs: +0 outside the shard.
__global__ __launch_bounds__(kBlock) void k_progress_frame(KParams P, float* __restrict__ rgb, const float2* __restrict__ mom,
                                                            float* __restrict__ var) {
    for (uint32_t s = blockIdx.x * kBlock + threadIdx.x; s < P.n_slots; s += gridDim.x * kBlock) {
        const SlotPixel pix = slot_pixel(P, s);
        const size_t at = (size_t)pix.col + (size_t)P.width * pix.row;
        const float* px = P.fb + 3 * at;
        const v3 mean = frame_mean(mk(px[0], px[1], px[2]), P.spp);
        rgb[3 * at] = mean.x, rgb[3 * at + 1] = mean.y, rgb[3 * at + 2] = mean.z;
        if (var) var[at] = frame_variance(mom[s], P.spp);
    }
}

hipError_t launch_resume(const KParams& P, uint32_t* list, uint32_t* count, uint32_t* count_other, uint32_t* req_count,
                         hipStream_t st) {
    const uint32_t blocks = (P.n_slots + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_resume, dim3(blocks), dim3(kBlock), 0, st, P, list, count, count_other, req_count);
    return hipGetLastError();
}

hipError_t launch_progress_finish(const KParams& P, hipStream_t st) {
    const uint32_t blocks = std::min<uint32_t>((P.n_slots + kBlock - 1) / kBlock, 2048u);
    hipLaunchKernelGGL(k_progress_finish, dim3(blocks), dim3(kBlock), 0, st, P);
    return hipGetLastError();
}

hipError_t launch_progress_frame(const KParams& P, float* rgb, const float2* mom, float* var, hipStream_t st) {
    const uint32_t blocks = std::min<uint32_t>((P.n_slots + kBlock - 1) / kBlock, 2048u);
    hipLaunchKernelGGL(k_progress_frame, dim3(blocks), dim3(kBlock), 0, st, P, rgb, mom, var);
    return hipGetLastError();
}

}  // namespace xrt
